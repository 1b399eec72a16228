// sm_iso3.hpp - iso_gemm on the bf16 MFMA with a 3-way split of the fp32 operands ("bf16x3"): the opt-in product of
// Iso-C's Newton-Schulz iteration.  The function is stated step by step in include/shardmerge_hip.h (smhip_iso_gemm,
// gemm = SMHIP_ISO_GEMM_BF16X3); IsoGemmParams, the tile enumeration, the edge rules and the four epilogues are
// iso_gemm's (sm_iso.hpp), unchanged.
//
//   iso_gemm3_nt   C = epilogue(A B^T), A [M x K] and B [N x K] fp32, both contiguous along k.
//   iso_gemm3_nn   C = epilogue(A B), A [M x K] contiguous along k, B [K x N] contiguous along n.
//                  An fp32 operand x is split while it is staged, between the global load and the LDS store:
//                  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16((x - x0) - x1), round to nearest even, both subtractions
//                  exact; x0 + x1 + x2 == x for 2^-100 <= |x| < 2^127.  HBM holds fp32 only and there is no pre-split
//                  pass.  Of the nine piece products six are kept - a0 b0, a0 b1, a1 b0, a1 b1, a0 b2, a2 b0 - each
//                  exact in fp32 (8 x 8 bits), all into ONE fp32 accumulator set on v_mfma_f32_32x32x16_bf16: lane
//                  (i, h) supplies k 8 h .. 8 h + 7 of row i, the C/D map is the fp32 instruction's.  The split of the
//                  work is iso_gemm's: four waves own 128 x 128 outputs, a wave 64 x 64 as 2 x 2 accumulator tiles of
//                  32 x 32, 64 registers; a k-block of 32 is 2 x 6 x 4 = 48 instructions a wave where the fp32 kernel
//                  issues 64.  Within an instruction group the small terms come first: a2 b0, a0 b2, a1 b1, a1 b0,
//                  a0 b1, a0 b0.
//                  LDS: three bf16 planes per operand, each [128][ISO3_PW = 20 dwords]: 32 k are 64 bytes, the row
//                  pitch is 80.  A lane reads 16 bytes, eight k of one row and one plane; the 16 lanes that share a
//                  pass read rows r .. r + 15 at the same k, and 80 r = 16 (5 r) with 5 odd puts them on 16 different
//                  16-byte bank groups (derived, not measured).  A k-contiguous piece of four k is split into two
//                  packed pairs per plane and leaves as one 8-byte store.  The n-contiguous B of the NN form is
//                  transposed on the way in: a thread loads the same four n at k and k + 1 (eight lanes cover 128
//                  contiguous bytes of a row of B), packs each n's pair per plane and stores one dword into row n -
//                  lanes that differ in n by 16 share a bank, a 2-way conflict (derived).  61440 bytes of LDS, single
//                  buffered: two work-groups fit a CU.
//                  Symmetric mode: off-diagonal tiles are mirrored as in iso_gemm.  Inside a diagonal tile (m, n) and
//                  (n, m) add a0 b1 and a1 b0 in swapped order and may differ in the last bit, so only m >= n is
//                  stored there and mirrored too: C == C^T bit for bit.
//                  The order of addition inside one bf16 MFMA instruction is not documented; the emulator branch fixes
//                  ascending k and, within a k, the order of the terms above, one rounded fp32 addition each.  The
//                  two are held to a bound (shardmerge_hip.h), not to each other.
#pragma once
#include "sm_iso.hpp"

namespace smhip {

constexpr int ISO3_BK = 32;                   // k per LDS stage: two instructions of 16 per term
constexpr int ISO3_PW = 20;                   // dwords per row of a plane: 16 of data (32 bf16), 4 of pad
constexpr int ISO3_PLANE = ISO_WG * ISO3_PW;  // dwords per plane
constexpr size_t ISO_GEMM3_LDS_BYTES = (size_t)2 * 3 * ISO3_PLANE * 4;

// the three bf16 pieces of x as fp32 values (the emulator's operands)
SM_HD void iso_split3(float x, float& x0, float& x1, float& x2) {
    x0 = bf16_to_f(f_to_bf16(x));
    const float r1 = x - x0;
    x1 = bf16_to_f(f_to_bf16(r1));
    x2 = bf16_to_f(f_to_bf16(r1 - x1));
}
// the pieces of two values, packed per plane (lo = a)
SM_HD void iso_split3_pair(float a, float b, uint32_t w[3]) {
    w[0] = pack_bf16x2(a, b);
    const float a1 = a - u2f(w[0] << 16), b1 = b - u2f(w[0] & 0xffff0000u);
    w[1] = pack_bf16x2(a1, b1);
    w[2] = pack_bf16x2(a1 - u2f(w[1] << 16), b1 - u2f(w[1] & 0xffff0000u));
}
// symmetric mode: a diagonal tile stores m >= n only, and every tile mirrors
SM_HD void iso_gemm3_put(const IsoGemmParams& p, int tm, int tn, int m, int n, float acc) {
    if (p.sym && tm == tn && m < n) return;
    const float v = iso_epilogue(p, m, n, acc);
    p.c[(size_t)m * p.ldc + n] = v;
    if (p.sym && m != n) p.c[(size_t)n * p.ldc + m] = v;
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef __bf16 iso3_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t iso3_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t iso3_u32x2 __attribute__((ext_vector_type(2)));
#endif

template <int FORM, class Ex>
SM_HD void k_iso_gemm3(Ex& ex, const IsoGemmParams& p) {
    int tm, tn;
    iso_tile(p, ex.bid(), tm, tn);
    const int m0 = tm * ISO_WG, n0 = tn * ISO_WG;
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, h = lane >> 5;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    uint32_t* As = (uint32_t*)ex.lds();
    uint32_t* Bs = As + 3 * ISO3_PLANE;
    iso_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    cf4 ra[4], rb[4];
    // the 1024 pieces of a k-contiguous tile are iso_gemm's: piece idx is row idx / 8, k 4 (idx % 8).  Piece r of the
    // n-contiguous tile belongs to item q = tid + 256 (r / 2): k pair (q / 8) % 16, its k 2 pair + r % 2, n 4 (q % 8 +
    // 8 (q / 128)) - a thread holds k and k + 1 of the same four n
    auto bk = [&](int r) { return 2 * (((tid + ISO_THREADS * (r >> 1)) >> 3) & 15) + (r & 1); };
    auto bn = [&](int r) { const int q = tid + ISO_THREADS * (r >> 1); return 4 * ((q & 7) + 8 * (q >> 7)); };
    const bool inner = m0 + ISO_WG <= p.M && n0 + ISO_WG <= p.N && p.avec && p.bvec;
    const float* pa[4];
    const float* pb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int idx = tid + ISO_THREADS * r;
        pa[r] = p.a + (size_t)(m0 + (idx >> 3)) * p.lda + 4 * (idx & 7);
        pb[r] = FORM == ISO_NT ? p.b + (size_t)(n0 + (idx >> 3)) * p.ldb + 4 * (idx & 7) : p.b + (size_t)bk(r) * p.ldb + n0 + bn(r);
    }
    auto load = [&](int k0) {
        if (inner && k0 + ISO3_BK <= p.K) {
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
            else rb[r] = iso_load4(p.b, p.ldb, p.K, p.N, k0 + bk(r), n0 + bn(r), p.bvec);
        }
    };
    // four k of one row: two packed pairs per plane, one 8-byte store each
    auto put4 = [&](uint32_t* t, int idx, const cf4& v) {
        uint32_t lo[3], hi[3];
        iso_split3_pair(v.x, v.y, lo);
        iso_split3_pair(v.z, v.w, hi);
        uint32_t* d = t + (idx >> 3) * ISO3_PW + 2 * (idx & 7);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const iso3_u32x2 w = {lo[pl], hi[pl]};
            *(iso3_u32x2*)(d + pl * ISO3_PLANE) = w;
        }
    };
    // k and k + 1 of four n: one packed pair per n and plane, into row n
    auto put_t = [&](int r, const cf4& even, const cf4& odd) {
        uint32_t* d = Bs + bn(r) * ISO3_PW + (bk(r) >> 1);
        const float e[4] = {even.x, even.y, even.z, even.w}, o[4] = {odd.x, odd.y, odd.z, odd.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t w[3];
            iso_split3_pair(e[j], o[j], w);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) d[pl * ISO3_PLANE + j * ISO3_PW] = w[pl];
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int r = 0; r < 4; ++r) put4(As, tid + ISO_THREADS * r, ra[r]);
        if (FORM == ISO_NT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) put4(Bs, tid + ISO_THREADS * r, rb[r]);
        } else {
            put_t(0, rb[0], rb[1]);
            put_t(2, rb[2], rb[3]);
        }
    };
    // instruction group j of the block: k 16 j + 8 h .. + 7 of this lane's rows, plane by plane
    auto frag = [&](const uint32_t* t, int row, int pl, int j) {
        return __builtin_bit_cast(iso3_bf16x8, *(const iso3_u32x4*)(t + pl * ISO3_PLANE + row * ISO3_PW + 8 * j + 4 * h));
    };
    auto step = [&](int j) {
        iso3_bf16x8 a[2][3], b[2][3];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                a[t][pl] = frag(As, wm + 32 * t + l32, pl, j);
                b[t][pl] = frag(Bs, wn + 32 * t + l32, pl, j);
            }
        // the small terms first; the four accumulator tiles of a term are independent instructions
        constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[x][TA[t]], b[y][TB[t]], acc[x][y], 0, 0, 0);
    };
    const int nkb = (p.K + ISO3_BK - 1) / ISO3_BK;
    load(0);
    for (int kb = 0; kb < nkb; ++kb) {
        stage();
        __syncthreads();
        if (kb + 1 < nkb) load(ISO3_BK * (kb + 1));
        step(0);
        if (p.K - ISO3_BK * kb > 16) step(1);
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
                if (m < p.M && n < p.N) iso_gemm3_put(p, tm, tn, m, n, acc[a][b][r]);
            }
#else
    // one output element at a time: ascending k, within a k the six terms in the order above, each an exact product and
    // one rounded fp32 addition (fmaf of an exact product)
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nthr = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int e = tid; e < ISO_WG * ISO_WG; e += nthr) {
            const int m = m0 + e / ISO_WG, n = n0 + e % ISO_WG;
            if (m >= p.M || n >= p.N) continue;
            const float* ar = p.a + (size_t)m * p.lda;
            float acc = 0.f;
            for (int k = 0; k < p.K; ++k) {
                float a0, a1, a2, b0, b1, b2;
                iso_split3(ar[k], a0, a1, a2);
                iso_split3(FORM == ISO_NT ? p.b[(size_t)n * p.ldb + k] : p.b[(size_t)k * p.ldb + n], b0, b1, b2);
                acc = fmaf(a2, b0, acc);
                acc = fmaf(a0, b2, acc);
                acc = fmaf(a1, b1, acc);
                acc = fmaf(a1, b0, acc);
                acc = fmaf(a0, b1, acc);
                acc = fmaf(a0, b0, acc);
            }
            iso_gemm3_put(p, tm, tn, m, n, acc);
        }
    });
#endif
}

// ---- kernel tags (sm_tag.hpp) and group 29 of smhip_side.hip (smhip_device.hpp) ----
// the LDS-staged bf16 MFMA GEMM on three-way split fp32 operands in its two forms (four waves of 2 x 2 accumulator tiles
// of 32 x 32, 64 registers)
SM_KERNEL_TAG_LB(KIsoGemm3NT, IsoGemmParams, "iso_gemm3_nt", k_iso_gemm3<ISO_NT>(ex, p), ISO_THREADS, 2)
SM_KERNEL_TAG_LB(KIsoGemm3NN, IsoGemmParams, "iso_gemm3_nn", k_iso_gemm3<ISO_NN>(ex, p), ISO_THREADS, 2)
#define SM_SIDE_KERNELS_29(X) X(KIsoGemm3NT) X(KIsoGemm3NN)

}  // namespace smhip
