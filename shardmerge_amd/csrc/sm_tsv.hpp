// sm_tsv.hpp - TSV merge (Gargiulo et al. 2025, "Task Singular Vectors: Reducing Task Interference in Model Merging"):
// the one kernel the operator adds to the primitives of sm_extract.hpp.  The function is stated step by step in
// include/shardmerge_hip.h (smhip_tsv_merge); its host path is DeltaHost::tsv_merge (sm_delta_host.hpp).
//
//   tsv_apply      out = base_out + lambda * B W^T on v_mfma_f32_16x16x4_f32, B [rows x Rp] and W [cols x Rp] fp32 panels
//                  (row pitches bp, wp >= Rp floats), Rp a multiple of 16 (0: the product is +0).  A work-group of four
//                  waves owns 128 x 128 outputs, a wave 64 x 64 of them: 4 x 4 accumulator tiles, 64 registers.  Both
//                  panels are contiguous along k, so a lane loads 4 consecutive k of its row (16 bytes: k0 + 4 g + j,
//                  g = lane >> 4) for both operands, and instruction j takes element j of the four lane groups.
//                  merged[m][n] is therefore ONE fp32 fmaf chain from +0 that, inside every block of 16 consecutive k,
//                  visits k0 + 4 g + j in the order j = 0..3 (outer), g = 0..3 (inner).  There is no k edge (Rp % 16 == 0);
//                  a row of B or W past the tensor's edge is not read and enters as +0 (its outputs are not stored).
//                  The epilogue reads base_out and writes out and delta_out one element at a time (element-aligned
//                  pointers, any rows and cols): out = round(fmaf(lambda, merged, fp32(base_out))), delta_out = merged.
//                  No LDS, no atomics.
#pragma once
#include "sm_extract.hpp"

namespace smhip {

constexpr int TSV_MAX_R = 256;                // k_active * r, and the width of the panels U, W and B
constexpr int TSV_WG = 128;                   // outputs per work-group along either axis
constexpr int TSV_WAVE = 64;                  // ... per wave

struct TsvApplyParams {
    const float* b;             // [rows x Rp], pitch bp
    const float* w;             // [cols x Rp], pitch wp
    int rows, cols, Rp, bp, wp;
    int pvec;                   // b, w 16-byte aligned and both pitches multiples of 4: 16-byte loads
    const void* base_out;
    int dtype;                  // of base_out and out
    float lambda;
    void* out;
    float* delta_out;           // may be null
    int gn;                     // work-groups along the columns; grid = gm * gn
};
// the position of k in the chain: inside a block of 16, k0 + 4 g + j comes at 4 j + g
SM_HD int tsv_chain_k(int pos) { return (pos & ~15) + 4 * (pos & 3) + ((pos >> 2) & 3); }
SM_HD void tsv_put(const TsvApplyParams& p, size_t idx, float merged) {
    lora_put(p.out, p.dtype, idx, fmaf(p.lambda, merged, load_elem(p.base_out, p.dtype, idx)));
    if (p.delta_out) p.delta_out[idx] = merged;
}

template <class Ex>
SM_HD void k_tsv_apply(Ex& ex, const TsvApplyParams& p) {
    const int tm = ex.bid() / p.gn, tn = ex.bid() % p.gn;
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int m0 = tm * TSV_WG + (wave >> 1) * TSV_WAVE, n0 = tn * TSV_WG + (wave & 1) * TSV_WAVE;
    if (m0 >= p.rows || n0 >= p.cols) return;              // (no barrier below)
    xl_f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[a][t] = xl_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* br[4];
    const float* wr[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int m = m0 + 16 * a + i16, n = n0 + 16 * a + i16;
        br[a] = m < p.rows ? p.b + (size_t)m * p.bp + 4 * g : nullptr;
        wr[a] = n < p.cols ? p.w + (size_t)n * p.wp + 4 * g : nullptr;
    }
    for (int k0 = 0; k0 < p.Rp; k0 += 16) {
        float bf[4][4], wf[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (p.pvec) {
                const cf4 zero = {0.f, 0.f, 0.f, 0.f};
                const cf4 x = br[a] ? *(const cf4*)(br[a] + k0) : zero, y = wr[a] ? *(const cf4*)(wr[a] + k0) : zero;
                bf[a][0] = x.x; bf[a][1] = x.y; bf[a][2] = x.z; bf[a][3] = x.w;
                wf[a][0] = y.x; wf[a][1] = y.y; wf[a][2] = y.z; wf[a][3] = y.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bf[a][j] = br[a] ? br[a][k0 + j] : 0.f;
                    wf[a][j] = wr[a] ? wr[a][k0 + j] : 0.f;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[a][j], wf[t][j], acc[a][t], 0, 0, 0);
    }
    // C/D map: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * a + 4 * g + r;
            if (m >= p.rows) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int n = n0 + 16 * t + i16;
                if (n < p.cols) tsv_put(p, (size_t)m * p.cols + n, acc[a][t][r]);
            }
        }
#else
    // the same chains, one output element at a time
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nthr = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int e = tid; e < TSV_WG * TSV_WG; e += nthr) {
            const int m = tm * TSV_WG + e / TSV_WG, n = tn * TSV_WG + e % TSV_WG;
            if (m >= p.rows || n >= p.cols) continue;
            const float* br = p.b + (size_t)m * p.bp;
            const float* wr = p.w + (size_t)n * p.wp;
            float acc = 0.f;
            for (int pos = 0; pos < p.Rp; ++pos) {
                const int k = tsv_chain_k(pos);
                acc = fmaf(br[k], wr[k], acc);
            }
            tsv_put(p, (size_t)m * p.cols + n, acc);
        }
    });
#endif
}

// ---- kernel tag (sm_tag.hpp) and group 12 of smhip_side.hip (smhip_device.hpp) ----
// base_out + lambda * B W^T on fp32 MFMA, four waves of 4 x 4 accumulator tiles (64 registers); everything before it runs
// on the kernels of the low-rank extraction
SM_KERNEL_TAG_LB(KTsvApply, TsvApplyParams, "tsv_apply", k_tsv_apply(ex, p), 256, 2)
#define SM_SIDE_KERNELS_12(X) X(KTsvApply)

}  // namespace smhip
