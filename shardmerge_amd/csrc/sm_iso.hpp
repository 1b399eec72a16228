// sm_iso.hpp - Iso-C merge (Marczak et al. 2025, "No Task Left Behind: Isotropic Model Merging with Common and
// Task-Specific Subspaces"): the task-arithmetic sum T of the deltas, taken as a matrix, with its spectrum replaced by
// its mean: merged = mean(S) U V^T.  U V^T is the orthogonal polar factor of T and mean(S) = <U V^T, T> / min(R, C), so
// the operator is a Newton-Schulz iteration: matrix products and nothing else.  The function is stated step by step in
// include/shardmerge_hip.h (smhip_iso_merge); its host path is DeltaHost::iso_merge (sm_delta_host.hpp).
//
//   iso_gemm_nt    C = epilogue(A B^T), A [M x K] and B [N x K] fp32, both contiguous along k.  With `sym` (A == B, or a
//                  B that is A's transpose bit for bit) only the tiles with tm >= tn are computed and every result is
//                  written to C[m][n] and C[n][m]: C == C^T bit for bit.
//   iso_gemm_nn    C = epilogue(A B), A [M x K] contiguous along k, B [K x N] contiguous along n.
//                  Both on v_mfma_f32_32x32x2_f32.  A work-group of four waves owns 128 x 128 outputs, a wave 64 x 64:
//                  2 x 2 accumulator tiles of 32 x 32, 64 registers.  k-blocks of 32 go through LDS: every thread loads
//                  four 16-byte pieces of each operand (coalesced along the operand's contiguous axis) into registers
//                  while the block before is multiplied, and stores them after the barrier.  A k-contiguous tile is
//                  [128][ISO_PA = 34] floats: lane (i, h) of an instruction reads [i][2 j + h], and 34 i + h takes 64
//                  distinct banks.  The n-contiguous B tile of the NN form is [32][ISO_PB = 160] floats: the two k of
//                  an instruction lie 160 = 32 (mod 64) banks apart.  37.9 KB of LDS, single buffered.
//                  Instruction j of a k-block takes k0 + 2 j from lanes 0..31 and k0 + 2 j + 1 from lanes 32..63, so
//                  every output element is ONE fp32 fmaf chain from +0 in ASCENDING k; when K is odd the chain ends
//                  with one step fmaf(+0, +0, acc), the empty half of the last instruction.  k is not split: the
//                  chain does not depend on the grid.  Rows of A or B past an edge enter as +0 and their outputs are
//                  not stored.  Any M, N, K >= 1 and element-aligned pitches; the 16-byte loads run when the operand's
//                  base is 16-byte aligned and its pitch a multiple of 4, piece by piece; a tile without an m or n edge
//                  loads its whole k-blocks without a test per piece.
//                  Epilogues, one rounded operation or one fmaf each: PLAIN acc | POLY fmaf(ca, acc, cb * E[m][n]) |
//                  AXPY fmaf(ca, E[m][n], acc) | CUBIC fmaf(ca, E[m][n], cb * acc).  No atomics.
//   iso_sum        T = sum_i alpha_i (finetune_i - base_i) in dare_merge's fp32 steps, one streaming pass.
//   iso_transpose  dst [cols x rows] = src [rows x cols]^T, 32 x 32 tiles through LDS.
//   iso_norm, iso_resid, iso_dot
//                  sum x^2 | sum (G_ij - [i == j])^2 | sum x y in fp64 in geo_gram's order: segments of 32768 elements,
//                  256 lanes that take the octets tid, tid + 256, ... of the segment, a binary tree through LDS; the
//                  segments are then added in index order by geo_gram_fold.
//   iso_scale      y = x * c.
//   iso_apply      merged = sigma * Q; out = round(fmaf(lambda, merged, fp32(base_out))); delta_out = merged.
#pragma once
#include "sm_tsv.hpp"

namespace smhip {

constexpr int ISO_MAX_S = 16384;              // min(rows, cols) at most
constexpr int ISO_MAX_ITER = 200;
constexpr int ISO_WG = 128;                   // outputs per work-group along either axis
constexpr int ISO_BK = 32;                    // k per LDS stage
constexpr int ISO_THREADS = 256;
constexpr int ISO_PA = 34;                    // floats per row of a k-contiguous tile [128][34]
constexpr int ISO_PB = 160;                   // floats per k of the n-contiguous tile [32][160]
constexpr size_t ISO_GEMM_LDS_FLOATS = (size_t)ISO_WG * ISO_PA + (ISO_WG * ISO_PA > ISO_BK * ISO_PB ? ISO_WG * ISO_PA : ISO_BK * ISO_PB);
enum { ISO_NT = 0, ISO_NN = 1 };
enum { ISO_EP_PLAIN = 0, ISO_EP_POLY = 1, ISO_EP_AXPY = 2, ISO_EP_CUBIC = 3 };
// the constants of the iteration (fp32, as hex floats): the quintic (a5, b5, c5) = (3.4445, -4.7750, 2.0315), the cubic
// (1.5, -0.5), and the residual above which the quintic runs
constexpr float ISO_A5 = 0x1.b8e56p+1f, ISO_B5 = -0x1.31999ap+2f, ISO_C5 = 0x1.040832p+1f;
constexpr float ISO_A3 = 0x1.8p+0f, ISO_B3 = -0x1p-1f;
constexpr double ISO_QUINTIC_ABOVE = 0x1.6666666666666p-2;    // 0.35

struct IsoGemmParams {
    const float* a;             // [M x K], pitch lda
    const float* b;             // NT: [N x K], NN: [K x N]; pitch ldb
    int M, N, K, lda, ldb;
    int avec, bvec;             // the operand's base is 16-byte aligned and its pitch a multiple of 4
    int sym;                    // NT only, M == N: tiles tm >= tn, mirrored
    int ep;
    float ca, cb;
    const float* e;             // [M x N], pitch lde (not PLAIN)
    int lde;
    float* c;                   // [M x N], pitch ldc
    int ldc;
    int gn;                     // work-groups along n (not sym); grid = gm * gn, sym: gm (gm + 1) / 2
};
SM_HD void iso_tile(const IsoGemmParams& p, int bid, int& tm, int& tn) {
    if (!p.sym) { tm = bid / p.gn; tn = bid % p.gn; return; }
    int t = 0;
    while ((t + 1) * (t + 2) / 2 <= bid) ++t;
    tm = t; tn = bid - t * (t + 1) / 2;
}
SM_HD float iso_epilogue(const IsoGemmParams& p, int m, int n, float acc) {
    if (p.ep == ISO_EP_PLAIN) return acc;
    const float e = p.e[(size_t)m * p.lde + n];
    if (p.ep == ISO_EP_POLY) return fmaf(p.ca, acc, aten_fmul_(p.cb, e));
    if (p.ep == ISO_EP_AXPY) return fmaf(p.ca, e, acc);
    return fmaf(p.ca, e, aten_fmul_(p.cb, acc));
}
SM_HD void iso_gemm_put(const IsoGemmParams& p, int tm, int tn, int m, int n, float acc) {
    const float v = iso_epilogue(p, m, n, acc);
    p.c[(size_t)m * p.ldc + n] = v;
    if (p.sym && tm != tn) p.c[(size_t)n * p.ldc + m] = v;
}
// elements (r, c .. c + 3) of x [nr x nc], +0 where there is none; c is a multiple of 4
SM_HD cf4 iso_load4(const float* x, int ld, int nr, int nc, int r, int c, int vec) {
    cf4 v = {0.f, 0.f, 0.f, 0.f};
    if (r >= nr || c >= nc) return v;
    const float* q = x + (size_t)r * ld + c;
    if (vec && c + 4 <= nc) return *(const cf4*)q;
    v.x = q[0];
    if (c + 1 < nc) v.y = q[1];
    if (c + 2 < nc) v.z = q[2];
    if (c + 3 < nc) v.w = q[3];
    return v;
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef float iso_f32x16 __attribute__((ext_vector_type(16)));
#endif

template <int FORM, class Ex>
SM_HD void k_iso_gemm(Ex& ex, const IsoGemmParams& p) {
    int tm, tn;
    iso_tile(p, ex.bid(), tm, tn);
    const int m0 = tm * ISO_WG, n0 = tn * ISO_WG;
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, h = lane >> 5;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    float* As = ex.lds();
    float* Bs = As + ISO_WG * ISO_PA;
    iso_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    cf4 ra[4], rb[4];
    // the 1024 pieces of a tile: piece idx of a k-contiguous tile is row idx / 8, k 4 (idx % 8); of the n-contiguous
    // tile k idx / 32, n 4 (idx % 32)
    // a tile with no m or n edge and both operands on the 16-byte path loads its whole k-blocks without a test per piece
    const bool inner = m0 + ISO_WG <= p.M && n0 + ISO_WG <= p.N && p.avec && p.bvec;
    const float* pa[4];
    const float* pb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int idx = tid + ISO_THREADS * r;
        pa[r] = p.a + (size_t)(m0 + (idx >> 3)) * p.lda + 4 * (idx & 7);
        pb[r] = FORM == ISO_NT ? p.b + (size_t)(n0 + (idx >> 3)) * p.ldb + 4 * (idx & 7) : p.b + (size_t)(idx >> 5) * p.ldb + n0 + 4 * (idx & 31);
    }
    auto load = [&](int k0) {
        if (inner && k0 + ISO_BK <= p.K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ra[r] = *(const cf4*)(pa[r] + k0);
                rb[r] = *(const cf4*)(FORM == ISO_NT ? pb[r] + k0 : pb[r] + (size_t)k0 * p.ldb);
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + ISO_THREADS * r;
            ra[r] = iso_load4(p.a, p.lda, p.M, p.K, m0 + (idx >> 3), k0 + 4 * (idx & 7), p.avec);
            if (FORM == ISO_NT) rb[r] = iso_load4(p.b, p.ldb, p.N, p.K, n0 + (idx >> 3), k0 + 4 * (idx & 7), p.bvec);
            else rb[r] = iso_load4(p.b, p.ldb, p.K, p.N, k0 + (idx >> 5), n0 + 4 * (idx & 31), p.bvec);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + ISO_THREADS * r;
            float* d = As + (idx >> 3) * ISO_PA + 4 * (idx & 7);
            d[0] = ra[r].x; d[1] = ra[r].y; d[2] = ra[r].z; d[3] = ra[r].w;
            float* f = FORM == ISO_NT ? Bs + (idx >> 3) * ISO_PA + 4 * (idx & 7) : Bs + (idx >> 5) * ISO_PB + 4 * (idx & 31);
            f[0] = rb[r].x; f[1] = rb[r].y; f[2] = rb[r].z; f[3] = rb[r].w;
        }
    };
    // instruction j of the block: k = 2 j + h of this lane's rows
    auto step = [&](int j) {
        const int kk = 2 * j + h;
        const float a0 = As[(wm + l32) * ISO_PA + kk], a1 = As[(wm + 32 + l32) * ISO_PA + kk];
        float b0, b1;
        if (FORM == ISO_NT) {
            b0 = Bs[(wn + l32) * ISO_PA + kk]; b1 = Bs[(wn + 32 + l32) * ISO_PA + kk];
        } else {
            b0 = Bs[kk * ISO_PB + wn + l32]; b1 = Bs[kk * ISO_PB + wn + 32 + l32];
        }
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    };
    const int nkb = (p.K + ISO_BK - 1) / ISO_BK;
    load(0);
    for (int kb = 0; kb < nkb; ++kb) {
        stage();
        __syncthreads();
        if (kb + 1 < nkb) load(ISO_BK * (kb + 1));
        const int left = p.K - ISO_BK * kb;
        if (left >= ISO_BK) {
#pragma unroll
            for (int j = 0; j < ISO_BK / 2; ++j) step(j);
        } else {
            for (int j = 0; j < (left + 1) / 2; ++j) step(j);
        }
        __syncthreads();
    }
    // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h, n = n0 + wn + 32 * b + l32;
                if (m < p.M && n < p.N) iso_gemm_put(p, tm, tn, m, n, acc[a][b][r]);
            }
#else
    // the same chains, one output element at a time
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nthr = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int e = tid; e < ISO_WG * ISO_WG; e += nthr) {
            const int m = m0 + e / ISO_WG, n = n0 + e % ISO_WG;
            if (m >= p.M || n >= p.N) continue;
            const float* ar = p.a + (size_t)m * p.lda;
            float acc = 0.f;
            if (FORM == ISO_NT) {
                const float* br = p.b + (size_t)n * p.ldb;
                for (int k = 0; k < p.K; ++k) acc = fmaf(ar[k], br[k], acc);
            } else {
                for (int k = 0; k < p.K; ++k) acc = fmaf(ar[k], p.b[(size_t)k * p.ldb + n], acc);
            }
            if (p.K & 1) acc = aten_fadd_(acc, 0.f);                // fmaf(+0, +0, acc): the last instruction's empty half
            iso_gemm_put(p, tm, tn, m, n, acc);
        }
    });
#endif
}

// ---- the sum of the weighted deltas ----
struct IsoSumParams {
    TiesInputs in;              // in.aligned: t included
    float alpha[TIES_MAX_MODELS];
    float* t;                   // [n]
    uint32_t* flags;            // [0]: bit i = finetune i has a non-finite delta
    int chunks;
};
template <class Ex>
SM_HD void k_iso_sum(Ex& ex, const IsoSumParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int k = p.in.k;
    ex.each(st, [&](int tid, EmptyState&) {
        uint32_t bad = 0;
        for (int q = 0; q < p.chunks; ++q) {
            Octet o;
            if (!octet_at(p.in, ex.bid(), ex.nthreads(), p.chunks, tid, q, o)) break;
            float b[8], S[8];
            delta_base8(p.in, o, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) S[e] = 0.f;
            for (int i = 0; i < k; ++i) {
                float f[8];
                delta_load8(p.in, i, o, b, f);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = f[e] - b[e];
                    if (delta_key(d) >= TIES_KEY_INF) bad |= 1u << i;
                    S[e] = aten_fadd_(S[e], aten_fmul_(d, p.alpha[i]));
                }
            }
            if (o.vec) {
                const cf4 w0 = {S[0], S[1], S[2], S[3]}, w1 = {S[4], S[5], S[6], S[7]};
                ((cf4*)p.t)[o.i0 / 4] = w0; ((cf4*)p.t)[o.i0 / 4 + 1] = w1;
            } else {
                for (int e = 0; e < o.cnt; ++e) p.t[o.i0 + e] = S[e];
            }
        }
        if (bad) ex.global_atomic_or_u32(p.flags, bad);
    });
}

// ---- the transposing copy ----
struct IsoTransposeParams {
    const float* src;           // [rows x cols]
    float* dst;                 // [cols x rows]
    int rows, cols;
    int gc;                     // tiles along the columns; grid = gr * gc
};
template <class Ex>
SM_HD void k_iso_transpose(Ex& ex, const IsoTransposeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int r0 = ex.bid() / p.gc * 32, c0 = ex.bid() % p.gc * 32;
    float* tile = ex.lds();                                         // [32][33]
    ex.each(st, [&](int tid, EmptyState&) {
        for (int j = 0; j < 4; ++j) {
            const int r = (tid >> 5) + 8 * j, c = tid & 31;
            if (r0 + r < p.rows && c0 + c < p.cols) tile[r * 33 + c] = p.src[(size_t)(r0 + r) * p.cols + c0 + c];
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int j = 0; j < 4; ++j) {
            const int c = (tid >> 5) + 8 * j, r = tid & 31;
            if (r0 + r < p.rows && c0 + c < p.cols) p.dst[(size_t)(c0 + c) * p.rows + r0 + r] = tile[r * 33 + c];
        }
    });
}

// ---- the ordered fp64 sums ----
enum { ISO_RED_NORM = 0, ISO_RED_RESID = 1, ISO_RED_DOT = 2 };
struct IsoReduceParams {
    const float* x;             // [n], 16-byte aligned
    const float* y;             // DOT: [n], 16-byte aligned
    size_t n;
    int s;                      // RESID: x is [s x s], contiguous
    double* part;               // [ceil(n / GEO_SEG_ELEMS)]
};
SM_HD size_t iso_reduce_lds_floats() { return LDS_SCRATCH_FLOATS + (size_t)2 * GEO_THREADS; }
template <int MODE, class Ex>
SM_HD void k_iso_reduce(Ex& ex, const IsoReduceParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();                                   // GEO_THREADS
    double* red = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const size_t start = (size_t)ex.bid() * GEO_SEG_ELEMS;
    const size_t len = p.n - start < GEO_SEG_ELEMS ? p.n - start : GEO_SEG_ELEMS;
    ex.each(st, [&](int tid, EmptyState&) {
        double acc = 0.0;
        for (size_t q = tid; q < segment_octets(len); q += nt) {
            const size_t i0 = start + 8 * q;
            const int cnt = (int)((len - 8 * q) < 8 ? (len - 8 * q) : 8);
            float x[8], y[8];
            if (cnt == 8) {
                load_elem8(p.x, DT_F32, i0, x);
                if (MODE == ISO_RED_DOT) load_elem8(p.y, DT_F32, i0, y);
            } else {
                for (int e = 0; e < 8; ++e) {
                    x[e] = e < cnt ? p.x[i0 + e] : 0.f;
                    if (MODE == ISO_RED_DOT) y[e] = e < cnt ? p.y[i0 + e] : 0.f;
                }
            }
            for (int e = 0; e < cnt; ++e) {
                if (MODE == ISO_RED_RESID) {
                    const size_t i = i0 + e;
                    const double d = geo_dadd((double)x[e], i / (size_t)p.s == i % (size_t)p.s ? -1.0 : 0.0);
                    acc = geo_dadd(acc, geo_dmul(d, d));
                } else {
                    // (the product of two fp32 values is exact in fp64: fused or not, this is ONE rounded addition)
                    acc = acc + (double)x[e] * (double)(MODE == ISO_RED_DOT ? y[e] : x[e]);
                }
            }
        }
        red[tid] = acc;
    });
    ex.sync();
    for (int s = nt >> 1; s > 0; s >>= 1) {
        ex.each(st, [&](int tid, EmptyState&) {
            if (tid < s) red[tid] = red[tid] + red[tid + s];
        });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0) p.part[ex.bid()] = red[0];
    });
}

// ---- y = x * c ----
struct IsoScaleParams {
    const float* x;             // [n], 16-byte aligned
    float* y;                   // [n], 16-byte aligned
    size_t n;
    float c;
};
template <class Ex>
SM_HD void k_iso_scale(Ex& ex, const IsoScaleParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t i = 4 * ((size_t)ex.bid() * ex.nthreads() + tid);
        if (i + 4 <= p.n) {
            const cf4 v = *(const cf4*)(p.x + i);
            const cf4 w = {aten_fmul_(v.x, p.c), aten_fmul_(v.y, p.c), aten_fmul_(v.z, p.c), aten_fmul_(v.w, p.c)};
            *(cf4*)(p.y + i) = w;
        } else {
            for (size_t j = i; j < p.n; ++j) p.y[j] = aten_fmul_(p.x[j], p.c);
        }
    });
}

// ---- the output ----
struct IsoApplyParams {
    const float* q;             // [n], 16-byte aligned: Q, oriented back
    float sigma, lambda;
    const void* base_out;
    int dtype;                  // of base_out and out
    void* out;
    float* delta_out;           // may be null
    size_t n;
    int aligned;                // base_out, out and delta_out are 16-byte aligned
    int chunks;
};
template <class Ex>
SM_HD void k_iso_apply(Ex& ex, const IsoApplyParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        for (int c = 0; c < p.chunks; ++c) {
            Octet o;
            if (!octet_at(0, p.n, p.aligned, ex.bid(), ex.nthreads(), p.chunks, tid, c, o)) break;
            float q[8], bo[8], r[8], M[8];
            ties_load8(p.q, DT_F32, o.i0, o.cnt, o.cnt == 8, q);
            ties_load8(p.base_out, p.dtype, o.i0, o.cnt, o.vec, bo);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                M[e] = aten_fmul_(p.sigma, q[e]);
                r[e] = fmaf(p.lambda, M[e], bo[e]);
            }
            ties_store8(p.out, p.dtype, p.delta_out, o.oi, o.cnt, o.vec, r, M);
        }
    });
}

// ---- kernel tags (sm_tag.hpp) and group 15 of smhip_side.hip (smhip_device.hpp) ----
// the LDS-staged fp32 MFMA GEMM in its two forms (four waves of 2 x 2 accumulator tiles of 32 x 32, 64 registers), the sum
// of the weighted deltas, the transposing copy, the three ordered fp64 sums, scale, apply
SM_KERNEL_TAG_LB(KIsoGemmNT, IsoGemmParams, "iso_gemm_nt", k_iso_gemm<ISO_NT>(ex, p), ISO_THREADS, 2)
SM_KERNEL_TAG_LB(KIsoGemmNN, IsoGemmParams, "iso_gemm_nn", k_iso_gemm<ISO_NN>(ex, p), ISO_THREADS, 2)
SM_KERNEL_TAG_LB(KIsoSum, IsoSumParams, "iso_sum", k_iso_sum(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KIsoTranspose, IsoTransposeParams, "iso_transpose", k_iso_transpose(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KIsoNorm, IsoReduceParams, "iso_norm", k_iso_reduce<ISO_RED_NORM>(ex, p), GEO_THREADS, 4)
SM_KERNEL_TAG_LB(KIsoResid, IsoReduceParams, "iso_resid", k_iso_reduce<ISO_RED_RESID>(ex, p), GEO_THREADS, 4)
SM_KERNEL_TAG_LB(KIsoDot, IsoReduceParams, "iso_dot", k_iso_reduce<ISO_RED_DOT>(ex, p), GEO_THREADS, 4)
SM_KERNEL_TAG_LB(KIsoScale, IsoScaleParams, "iso_scale", k_iso_scale(ex, p), 256, 4)
SM_KERNEL_TAG_LB(KIsoApply, IsoApplyParams, "iso_apply", k_iso_apply(ex, p), 256, 4)
#define SM_SIDE_KERNELS_15(X) X(KIsoGemmNT) X(KIsoGemmNN) X(KIsoSum) X(KIsoTranspose) X(KIsoNorm) X(KIsoResid) X(KIsoDot) X(KIsoScale) X(KIsoApply)

}  // namespace smhip
