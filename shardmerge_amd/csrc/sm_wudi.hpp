// sm_wudi.hpp - WUDI-Merging (Cheng et al. 2025, "Whoever Started the Interference Should End It: Guiding Data-Free Model
// Merging via Task Vectors"): per linear layer the merged task vector X minimises the interference
// L(X) = sum_i ||(X - d_i) d_i^T||_F^2 / ||d_i||_F^2 with the task vectors d_i [R x C] themselves standing in for the
// layer's inputs.  grad L = 2 (X S - P), S = sum_i d_i^T d_i / n_i [C x C], P = sum_i d_i (d_i^T d_i) / n_i [R x C]: S and P
// are built once, and a step is ONE product X S plus an Adam update.  The function is stated step by step in
// include/shardmerge_hip.h (smhip_wudi_merge); its host path is DeltaHost::wudi_merge (sm_delta_host.hpp).
//
// Three LDS-staged GEMM kernels on v_mfma_f32_32x32x2_f32 with iso_gemm's split of the work: a work-group of four waves
// owns 128 x 128 outputs, a wave 2 x 2 accumulator tiles of 32 x 32 (64 registers); k-blocks of 32 go through LDS, loaded
// into registers while the block before is multiplied; lane half h of instruction j supplies k = 2 j + h, so every output
// is ONE fp32 fmaf chain from +0 in ASCENDING k, ended by fmaf(+0, +0, acc) when the length is odd; k is not split.  Rows
// and columns past an edge enter as +0 and their outputs are not stored.  A task vector is never stored: where a kernel
// reads one, it loads the finetune and its base (16-bit or fp32) in 16-byte pieces of 8 (fp32: twice 4) elements along the
// columns, subtracts in registers and stores fp32 to LDS.
//
//   wudi_gram   the TN form, D^T D with the contraction along the ROWS of D.  Both operand tiles are k-major: [32][WUDI_PK
//               = 160] floats, 32 rows of D by 128 of its columns - the global loads run along the columns and the LDS
//               stores are rows of 8 floats; lane (i, h) reads [2 j + h][i], and 160 = 32 (mod 64) puts the two k of an
//               instruction into different bank halves.  Only the tiles ta >= tb are computed, a diagonal tile stages ONE
//               operand.  Epilogue: Sh = fmul(w, acc) to [a][b] and [b][a], and S = Sh (the first task) or fadd(S, Sh)
//               to both, in the same pass: Sh == Sh^T and S == S^T bit for bit.  40 KB of LDS.
//   wudi_rhs    P (+)= D Sh.  The A tile is k-contiguous, [128][ISO_PA = 34], formed from finetune and base at staging (an
//               octet is 8 consecutive k of one row); B is the symmetric Sh read as the NT form reads it (row n, k
//               contiguous).  Epilogue: store, or fadd into P.
//   wudi_step   X S in the NT form (S == S^T bit for bit) with the Adam update as its epilogue: per output element it
//               reads P, m, v, X and writes m, v, X' - and g when asked, on the two steps whose gradient is reported -
//               instead of a GEMM output and a separate optimiser pass.  X' is another buffer than X: other work-groups
//               still read X as an operand.  The C/D map gives every plane access 128-byte runs along n.
// No atomics; the kernels hold no scratch (python tools/resource_report.py side26).
#pragma once
#include "sm_iso.hpp"

namespace smhip {

constexpr int WUDI_MAX_C = 32768;             // columns at most: S and Sh are [C x C]
constexpr int WUDI_MAX_ITER = 2000;
constexpr int WUDI_PK = 160;                  // floats per k of a k-major tile [32][160]
constexpr size_t WUDI_LDS_FLOATS = 2 * (ISO_WG * ISO_PA > ISO_BK * WUDI_PK ? ISO_WG * ISO_PA : ISO_BK * WUDI_PK);
// Adam's constants (fp32, as hex floats): 0.9, 0.999, 1e-8
constexpr float WUDI_B1 = 0x1.ccccccp-1f, WUDI_B2 = 0x1.ff7ceep-1f, WUDI_EPS = 0x1.5798eep-27f;
enum { WUDI_GRAM = 0, WUDI_RHS = 1, WUDI_STEP = 2 };

// a task vector d = fp32(finetune) - fp32(base) [nr x nc], rows `ld` elements apart
struct WudiDelta {
    const void* ft;
    const void* base;
    int dtype, ld;
    int nr, nc;
    int vec;                    // both pointers are 16-byte aligned and the pitch is a multiple of 8 (fp32: 4)
};
struct WudiGemmParams {
    int M, N, K;                // gram: M = N = d.nc, K = d.nr; rhs: M = d.nr, K = d.nc; step: a [M x K]
    WudiDelta d;                // gram, rhs
    const float* a;             // step: X [M x K], pitch lda
    const float* b;             // rhs: Sh, step: S [N x K], pitch ldb - symmetric bit for bit in the merge (N == K)
    int lda, ldb, avec, bvec;   // vec: the base is 16-byte aligned and the pitch a multiple of 4
    int first;                  // gram, rhs: the first task stores, the later ones fadd
    float w;                    // gram
    float* sh;                  // gram: [N x N], pitch ldo
    float* s;                   // gram: [N x N], pitch ldo
    int ldo;
    float* p;                   // rhs: out, step: in; [M x N], pitch ldp like m, v, xn, g
    float* m;                   // step: Adam's moments, updated in place
    float* v;
    const float* x;             // step: X as the update reads it, [M x N], pitch ldx (the merge: a, N == K)
    int ldx;
    float* xn;                  // step: X'
    float* g;                   // step: the gradient, or null
    int ldp;
    float c1, c2, st, qt;       // step: fp32(1 - 0.9), fp32(1 - 0.999), s_t, q_t
    int gn;                     // rhs, step: work-groups along n; grid = gm * gn.  gram: grid = gn (gn + 1) / 2
};

// elements (r, c .. c + 7) of the task vector, +0 where there is none; c is a multiple of 8
SM_HD void wudi_delta8(const WudiDelta& s, int r, int c, float* d) {
    if (r >= s.nr || c >= s.nc) {
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = 0.f;
        return;
    }
    const size_t i0 = (size_t)r * s.ld + c;
    const int cnt = s.nc - c < 8 ? s.nc - c : 8;
    float f[8], b[8];
    ties_load8(s.ft, s.dtype, i0, cnt, s.vec && cnt == 8, f);
    ties_load8(s.base, s.dtype, i0, cnt, s.vec && cnt == 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = f[e] - b[e];
}
// ... of a piece that lies inside the task vector, on the 16-byte path
SM_HD void wudi_delta8_inner(const WudiDelta& s, int r, int c, float* d) {
    const size_t i0 = (size_t)r * s.ld + c;
    float f[8], b[8];
    load_elem8(s.ft, s.dtype, i0, f);
    load_elem8(s.base, s.dtype, i0, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = f[e] - b[e];
}
SM_HD float wudi_delta1(const WudiDelta& s, int r, int c) {
    const size_t i = (size_t)r * s.ld + c;
    return load_elem(s.ft, s.dtype, i) - load_elem(s.base, s.dtype, i);
}
// tile bid of the lower triangle, row after row: ta >= tb
SM_HD void wudi_tri(int bid, int& ta, int& tb) {
    int t = 0;
    while ((t + 1) * (t + 2) / 2 <= bid) ++t;
    ta = t; tb = bid - t * (t + 1) / 2;
}
SM_HD float wudi_fsub(float a, float b) { return aten_fadd_(a, -b); }

// what a kernel does with the finished chain of output (m, n)
template <int KIND>
SM_HD void wudi_put(const WudiGemmParams& p, int tm, int tn, int m, int n, float acc) {
    if (KIND == WUDI_GRAM) {
        const size_t i = (size_t)m * p.ldo + n, j = (size_t)n * p.ldo + m;
        const float sh = aten_fmul_(p.w, acc);
        const float s = p.first ? sh : aten_fadd_(p.s[i], sh);
        p.sh[i] = sh; p.s[i] = s;
        if (tm != tn) { p.sh[j] = sh; p.s[j] = s; }
    } else if (KIND == WUDI_RHS) {
        const size_t i = (size_t)m * p.ldp + n;
        p.p[i] = p.first ? acc : aten_fadd_(p.p[i], acc);
    } else {
        const size_t i = (size_t)m * p.ldp + n;
        const float g = aten_fmul_(2.f, wudi_fsub(acc, p.p[i]));
        const float m1 = fmaf(WUDI_B1, p.m[i], aten_fmul_(p.c1, g));
        const float v1 = fmaf(WUDI_B2, p.v[i], aten_fmul_(aten_fmul_(p.c2, g), g));
        const float den = aten_fadd_(aten_fmul_(sqrtf(v1), p.qt), WUDI_EPS);
        const float q = m1 / den;
        p.m[i] = m1; p.v[i] = v1;
        p.xn[i] = wudi_fsub(p.x[(size_t)m * p.ldx + n], aten_fmul_(p.st, q));
        if (p.g) p.g[i] = g;
    }
}

template <int KIND, class Ex>
SM_HD void k_wudi_gemm(Ex& ex, const WudiGemmParams& p) {
    int tm, tn;
    if (KIND == WUDI_GRAM) wudi_tri(ex.bid(), tm, tn);
    else { tm = ex.bid() / p.gn; tn = ex.bid() % p.gn; }
    const int m0 = tm * ISO_WG, n0 = tn * ISO_WG;
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, h = lane >> 5;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const bool diag = KIND == WUDI_GRAM && tm == tn;
    float* As = ex.lds();
    float* Bs = KIND == WUDI_GRAM ? (diag ? As : As + ISO_BK * WUDI_PK) : As + ISO_WG * ISO_PA;
    iso_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // the pieces of a k-block held in registers while the block before is multiplied.  A task-vector tile is 512 octets,
    // two per thread: octet idx of a k-major tile is k idx / 16, column 8 (idx % 16); of a k-contiguous tile row idx / 4,
    // k 8 (idx % 4).  An fp32 k-contiguous tile is iso_gemm's: 1024 pieces of 4, row idx / 8, k 4 (idx % 8).
    float da[2][8], db[2][8];
    cf4 ra[4], rb[4];
    // a tile with no m or n edge and every operand on the 16-byte path loads its whole k-blocks without a test per piece
    const bool inner = m0 + ISO_WG <= p.M && n0 + ISO_WG <= p.N && (KIND == WUDI_STEP ? p.avec : p.d.vec) && (KIND == WUDI_GRAM || p.bvec);
    auto load = [&](int k0) {
        if (inner && k0 + ISO_BK <= p.K) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int idx = tid + ISO_THREADS * r;
                if (KIND == WUDI_GRAM) {
                    wudi_delta8_inner(p.d, k0 + (idx >> 4), m0 + 8 * (idx & 15), da[r]);
                    if (!diag) wudi_delta8_inner(p.d, k0 + (idx >> 4), n0 + 8 * (idx & 15), db[r]);
                }
                if (KIND == WUDI_RHS) wudi_delta8_inner(p.d, m0 + (idx >> 2), k0 + 8 * (idx & 3), da[r]);
            }
            if (KIND != WUDI_GRAM) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int idx = tid + ISO_THREADS * r;
                    if (KIND == WUDI_STEP) ra[r] = *(const cf4*)(p.a + (size_t)(m0 + (idx >> 3)) * p.lda + k0 + 4 * (idx & 7));
                    rb[r] = *(const cf4*)(p.b + (size_t)(n0 + (idx >> 3)) * p.ldb + k0 + 4 * (idx & 7));
                }
            }
            return;
        }
        if (KIND == WUDI_GRAM) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int idx = tid + ISO_THREADS * r;
                wudi_delta8(p.d, k0 + (idx >> 4), m0 + 8 * (idx & 15), da[r]);
                if (!diag) wudi_delta8(p.d, k0 + (idx >> 4), n0 + 8 * (idx & 15), db[r]);
            }
            return;
        }
        if (KIND == WUDI_RHS) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int idx = tid + ISO_THREADS * r;
                wudi_delta8(p.d, m0 + (idx >> 2), k0 + 8 * (idx & 3), da[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + ISO_THREADS * r;
            if (KIND == WUDI_STEP) ra[r] = iso_load4(p.a, p.lda, p.M, p.K, m0 + (idx >> 3), k0 + 4 * (idx & 7), p.avec);
            rb[r] = iso_load4(p.b, p.ldb, p.N, p.K, n0 + (idx >> 3), k0 + 4 * (idx & 7), p.bvec);
        }
    };
    auto stage = [&]() {
        if (KIND != WUDI_STEP) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int idx = tid + ISO_THREADS * r;
                const int at = KIND == WUDI_GRAM ? (idx >> 4) * WUDI_PK + 8 * (idx & 15) : (idx >> 2) * ISO_PA + 8 * (idx & 3);
#pragma unroll
                for (int e = 0; e < 8; ++e) As[at + e] = da[r][e];
                if (KIND == WUDI_GRAM && !diag) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) Bs[at + e] = db[r][e];
                }
            }
        }
        if (KIND != WUDI_GRAM) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int idx = tid + ISO_THREADS * r;
                const int at = (idx >> 3) * ISO_PA + 4 * (idx & 7);
                if (KIND == WUDI_STEP) { As[at] = ra[r].x; As[at + 1] = ra[r].y; As[at + 2] = ra[r].z; As[at + 3] = ra[r].w; }
                Bs[at] = rb[r].x; Bs[at + 1] = rb[r].y; Bs[at + 2] = rb[r].z; Bs[at + 3] = rb[r].w;
            }
        }
    };
    // instruction j of the block: k = 2 j + h of this lane's rows
    auto step = [&](int j) {
        const int kk = 2 * j + h;
        float a0, a1, b0, b1;
        if (KIND == WUDI_GRAM) {
            a0 = As[kk * WUDI_PK + wm + l32]; a1 = As[kk * WUDI_PK + wm + 32 + l32];
            b0 = Bs[kk * WUDI_PK + wn + l32]; b1 = Bs[kk * WUDI_PK + wn + 32 + l32];
        } else {
            a0 = As[(wm + l32) * ISO_PA + kk]; a1 = As[(wm + 32 + l32) * ISO_PA + kk];
            b0 = Bs[(wn + l32) * ISO_PA + kk]; b1 = Bs[(wn + 32 + l32) * ISO_PA + kk];
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
                if (m < p.M && n < p.N) wudi_put<KIND>(p, tm, tn, m, n, acc[a][b][r]);
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
            float acc = 0.f;
            for (int k = 0; k < p.K; ++k) {
                if (KIND == WUDI_GRAM) acc = fmaf(wudi_delta1(p.d, k, m), wudi_delta1(p.d, k, n), acc);
                else if (KIND == WUDI_RHS) acc = fmaf(wudi_delta1(p.d, m, k), p.b[(size_t)n * p.ldb + k], acc);
                else acc = fmaf(p.a[(size_t)m * p.lda + k], p.b[(size_t)n * p.ldb + k], acc);
            }
            if (p.K & 1) acc = aten_fadd_(acc, 0.f);                // fmaf(+0, +0, acc): the last instruction's empty half
            wudi_put<KIND>(p, tm, tn, m, n, acc);
        }
    });
#endif
}

// ---- kernel tags (sm_tag.hpp) and group 26 of smhip_side.hip (smhip_device.hpp) ----
// the three GEMMs of WUDI-Merging: four waves of 2 x 2 accumulator tiles of 32 x 32, 64 registers
SM_KERNEL_TAG_LB(KWudiGram, WudiGemmParams, "wudi_gram", k_wudi_gemm<WUDI_GRAM>(ex, p), ISO_THREADS, 2)
SM_KERNEL_TAG_LB(KWudiRhs, WudiGemmParams, "wudi_rhs", k_wudi_gemm<WUDI_RHS>(ex, p), ISO_THREADS, 2)
SM_KERNEL_TAG_LB(KWudiStep, WudiGemmParams, "wudi_step", k_wudi_gemm<WUDI_STEP>(ex, p), ISO_THREADS, 2)
#define SM_SIDE_KERNELS_26(X) X(KWudiGram) X(KWudiRhs) X(KWudiStep)

}  // namespace smhip
