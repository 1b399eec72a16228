// sm_kernels.hpp - the transform passes of the spectral-merge pipeline, the kernels that exist once per plan:
// F1, F1Q, F2, F2S, I1, I2 (with the _r1 forms of the column passes) and the one-work-group 1-D pair merge.
// The selection and reduction kernels: sm_select.hpp; the blend, norm and layout kernels: sm_merge.hpp; neither is used here.
//
// Each body is a template over an execution policy `Ex`:
//   * DeviceExec (smhip_device.hpp) -> a real gfx950 work-group, `each` runs the
//     lambda once for threadIdx.x and `sync` is s_barrier;
//   * HostExec (tests/emul)       -> a sequential CPU emulation of one
//     work-group, used by the "not gpu" tests to check indexing.
// Pipeline for one pair-merge of two real [R x C] tensors a, b:
//   F1  rows:    z = a + i b, C-point FFT per row, split by Hermitian symmetry
//                into half-spectra A_row, B_row -> T1[R][Cb] (float4 per bin)
//   F2  columns: R-point FFT per bin column of A and B -> planes [Cb][R]:
//                Re Fa, Im Fa, Re Fb (normalised), + level-1 histogram
//   SEL select:  exact k-th order statistic by 3-level radix histograms
//   RED / BLEND: masked slerp sums, class blend -> Re R plane (+ cull histogram)
//   I1  columns: inverse R-point FFT of (Re R culled, Im Fa) -> G[R][Cb]
//   I2  rows:    two rows per transform (two-for-one), inverse C-point FFT,
//                scale, NaN/Inf policy, add base, bf16 store
#pragma once
#include "sm_common.hpp"
#include "sm_tag.hpp"
#include "sm_aten_core.hpp"

namespace smhip {

// =====================================================================
// F1: forward row pass
// =====================================================================
// rows_first: the row passes of several raw deltas in ONE launch.  The deltas of a layer share their base, so the
// work-groups that transform the same rows of different signals are placed on one XCD, next to each other in dispatch
// order (xcd_remap): the base rows come from HBM once and out of that L2 afterwards (the row pass with its base rows
// always in cache runs 11 % faster: 462 against 520 us per 28672x8192 signal).
constexpr int F1_MAX_SIGS = 16;
struct F1Sigs {
    int n;                              // <= 1: off (the kernel uses a, b, t1, partials)
    const void* x[F1_MAX_SIGS];         // signal s: a.x (b.x = a.x + b_off bytes: row-pair mode)
    const void* base[F1_MAX_SIGS];      // its base (b.base likewise) or null
    cf4* t1[F1_MAX_SIGS];
    double* partials[F1_MAX_SIGS];
    long long b_off;
};
// work-group `wg` of a launch over sg.n signals -> its signal and its block id within that signal's grid (XG: the
// work-groups of ONE signal that share lines of T1 and must stay adjacent, see k_f1)
SM_HD int pick_signal(int n, int wg, int XG, int& sig) {
    sig = 0;
    if (n <= 1) return XG > 1 ? xcd_remap(wg, XG) : wg;
    const int G = XG * n;
    const int L = xcd_remap(wg, G);
    const int r = L % G;
    sig = r / XG;
    return (L / G) * XG + r % XG;
}
SM_HD int f1_pick_signal(const F1Sigs& sg, int wg, int XG, int& sig) { return pick_signal(sg.n, wg, XG, sig); }

struct F1Params {
    FftPlanDev plan;       // N = C
    SigDesc a, b;
    int R, C, Cb;
    int pitch4;            // T1 row pitch in float4
    int ilv;               // rows interleaved in T1 (1 or 2): element (r, k) at ((r/ilv)*pitch4 + k)*ilv + r%ilv
    int nb;                // rows (transforms) per work-group
    size_t row_stride;     // elements between consecutive transforms' inputs (C; 2C in row-pair mode,
                           // where "a" is row 2m and "b" row 2m+1 of ONE tensor: b's pointers are a's + C)
    int vec;               // 1: C % 8 == 0 and 16-byte aligned inputs
    cf4* t1;               // the column pass reads ilv*16 contiguous bytes per (row group, bin)
    double* partials;      // [grid][2]: sum a^2, sum b^2 of this work-group
    // k_f1q only (radix-4 column step folded into the row pass):
    int R2;                // transforms per slab: work-group w handles "rows" w + g*R2, g = 0..3
    int rowpair;           // 1: row-pair mode (a = row 2w, b = row 2w+1 of one tensor; row_stride = 2C)
    int Rcol;              // column length R (the folded twiddles are W_R)
    size_t slab_elems;     // float4 per k1 slab of T1
    const cf2* twR;        // exp(-2 pi i j / R), j < R
    F1Sigs sigs;           // k_f1 / k_f1q: several signals in one launch
    AtenFuse fuse;         // norm_mode = reference_cpu: the deltas' torch.norm summaries come out of this pass (prefix = null: off)
    int fuse_rowpair;      // 1: signal = the launch's signal index, matrix row = 2 * unit + component; 0: signal = component (K = 2)
};

template <class P> constexpr bool f1_full_batch() {
    if constexpr (P::is_static) return P::T <= 256; else return false;
}
// paired (packed-f32) butterflies cost registers: the 512/1024-thread row plans, compiled for
// 128 VGPRs, spill with them (14336: 76 bytes of scratch -> 0, -21 % time) and stay scalar
#ifndef SM_ROW_PACK_MAX_T
#define SM_ROW_PACK_MAX_T 256
#endif
template <class P> constexpr bool f1_opaque() {
    if constexpr (P::is_static) return P::T >= 512; else return false;
}
// ... (PACK mode of wg_fft: 0 single floats, 1 paired butterflies, 2 complex-packed - the scalar form's register count)
#ifndef SM_ROW_PACK_BIG
#define SM_ROW_PACK_BIG 0
#endif
template <class P> constexpr int f1_pack() {
    if constexpr (P::is_static) return P::T <= SM_ROW_PACK_MAX_T ? 1 : SM_ROW_PACK_BIG; else return 1;
}

template <class P, class Ex>
SM_HD void k_f1(Ex& ex, const F1Params& p) {
    typename Ex::template State<FftState> st;
    ex.init(st);
    float* lds = ex.lds() + LDS_SCRATCH_FLOATS;
    const FftPlanDev& pl = p.plan;
    const int T = plan_T<P>(pl), C = plan_N<P>(pl);
    const int LF = plan_lds<P>(pl);
    // the work-groups of an interleaved row group fill the same 128-byte lines: they sit
    // on one XCD, adjacent in dispatch order, so the partial-line writes merge in that L2
    int sig_;
    const int bid = f1_pick_signal(p.sigs, ex.bid(), (p.ilv > p.nb) ? p.ilv / p.nb : 1, sig_);
    const int pbid = p.sigs.n > 1 ? bid : ex.bid();
    SigDesc sgA = p.a, sgB = p.b;
    cf4* t1_ = p.t1;
    double* partials_ = p.partials;
    if (p.sigs.n > 1) {
        sgA.x = p.sigs.x[sig_]; sgA.base = p.sigs.base[sig_];
        sgB.x = (const char*)sgA.x + p.sigs.b_off; sgB.base = sgA.base ? (const char*)sgA.base + p.sigs.b_off : nullptr;
        t1_ = p.sigs.t1[sig_]; partials_ = p.sigs.partials[sig_];
    }
    // static plans are launched only when the 16-byte vector path applies (host checks),
    // so the element-wise path is not even compiled into them
    const bool vec = P::is_static ? true : (p.vec != 0);
    // norm_mode = reference_cpu, fused summaries: which (signal, matrix row) region g holds in component comp
    auto fuse_where = [&](int comp) {
        return [&, comp](int g, int& sig, long long& mrow) {
            const int row = bid * p.nb + g;
            if (row >= p.R) return false;
            if (p.fuse_rowpair) { sig = sig_; mrow = 2LL * row + comp; }
            else { sig = comp; mrow = row; if (comp == 1 && !sgB.x) return false; }
            return true;
        };
    };
    if constexpr (P::is_static) {
        if constexpr (aten_fusable(P::N, P::T)) {
            if (p.fuse.prefix) ex.each(st, [&](int tid, FftState& s) {
                s.fep[0] = aten_fused_ep<P::N, P::T>(p.fuse, tid, fuse_where(0));
                s.fep[1] = aten_fused_ep<P::N, P::T>(p.fuse, tid, fuse_where(1));
            });
        }
    }

    ex.each(st, [&](int tid, FftState& s) {
        const int g = tid / T, t = tid % T;
        const int row = bid * p.nb + g;
        const bool valid = row < p.R;
        double sa = 0.0, sb = 0.0;
        if (vec && sgA.dtype != DT_F32 && sgB.dtype != DT_F32) {
            // 16-bit inputs (the merge itself): all 16-byte loads of the row are issued back
            // to back - no load sits inside a divergent branch, out-of-range ones are
            // clamped to element 0 and masked afterwards - and only then decoded
            constexpr int NQ = EMAX / 8;
            u32x4 ra[NQ], rab[NQ], rb[NQ], rbb[NQ];
            bool ok[NQ];
            size_t off[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int n0 = 8 * (t + q * T);
                ok[q] = valid && n0 < C;
                off[q] = ok[q] ? ((size_t)row * p.row_stride + n0) / 8 : 0;
            }
            // an absent operand reads a's values instead (always there) and is masked out below
            const bool has_ab = sgA.base != nullptr, has_b = sgB.x != nullptr, has_bb = has_b && sgB.base != nullptr;
            const u32x4* pa = (const u32x4*)sgA.x;
            const u32x4* pab = has_ab ? (const u32x4*)sgA.base : pa;
            const u32x4* pb = has_b ? (const u32x4*)sgB.x : pa;
            const u32x4* pbb = has_bb ? (const u32x4*)sgB.base : pa;
            // the 128-VGPR variants (512/1024-thread work-groups, run-time plans) keep half of the
            // row's loads in flight at a time: all sixteen at once made them spill
            constexpr int QB = f1_full_batch<P>() ? NQ : NQ / 2;
            bool all_ok = true;
#pragma unroll
            for (int q = 0; q < NQ; ++q) all_ok = all_ok && ok[q];
            static_for<0, NQ / QB>([&](auto h_c) {
            constexpr int Q0 = decltype(h_c)::value * QB, Q1 = Q0 + QB;
#pragma unroll
            for (int q = Q0; q < Q1; ++q) ra[q] = pa[off[q]];
#pragma unroll
            for (int q = Q0; q < Q1; ++q) rab[q] = pab[off[q]];
#pragma unroll
            for (int q = Q0; q < Q1; ++q) rb[q] = pb[off[q]];
#pragma unroll
            for (int q = Q0; q < Q1; ++q) rbb[q] = pbb[off[q]];
            // MASKED: some loads of this thread were clamped (ragged row tail, padded grid)
            auto decode = [&](auto masked_c) {
                constexpr bool MASKED = decltype(masked_c)::value;
#pragma unroll
                for (int q = Q0; q < Q1; ++q) {
                    float va[8], vb[8], ba[8], bb[8];
                    decode16x8(ra[q], sgA.dtype, va);
                    decode16x8(rab[q], sgA.dtype, ba);
                    decode16x8(rb[q], sgB.dtype, vb);
                    decode16x8(rbb[q], sgB.dtype, bb);
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        if (!has_ab) ba[c] = 0.f;
                        if (!has_b) vb[c] = 0.f;
                        if (!has_bb) bb[c] = 0.f;
                    }
                    float pa = 0.f, pb = 0.f;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        float xa = (va[c] - ba[c]) * sgA.prescale;
                        float xb = (vb[c] - bb[c]) * sgB.prescale;
                        if (MASKED && !ok[q]) { xa = 0.f; xb = 0.f; }      // never NaN * 0 from a clamped load
                        s.xr[q * 8 + c] = xa; s.xi[q * 8 + c] = xb;
                        pa += xa * xa; pb += xb * xb;
                    }
                    sa += pa; sb += pb;
                }
            };
            if (all_ok) decode(std::false_type{});
            else decode(std::true_type{});
            });

        } else if (vec) {
            // any other dtype mix (later tournament rounds: an fp32 intermediate against a raw
            // bf16 delta): one signal at a time, its loads issued together, decoded afterwards
            constexpr int NQ = EMAX / 8;
            bool ok[NQ];
            size_t off[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int n0 = 8 * (t + q * T);
                ok[q] = valid && n0 < C;
                off[q] = ok[q] ? (size_t)row * p.row_stride + n0 : 0;
            }
            auto load_signal = [&](const SigDesc& sg, float* dst, double& ss) {
                if (!sg.x) {
#pragma unroll
                    for (int i = 0; i < 8 * NQ; ++i) dst[i] = 0.f;
                    return;
                }
                const bool has_base = sg.base != nullptr;
                float v[NQ][8], bv[NQ][8];
                if (sg.dtype == DT_F32) {
                    const cf4* px = (const cf4*)sg.x;
                    const cf4* pb = has_base ? (const cf4*)sg.base : px;
                    cf4 r[NQ][2], rb[NQ][2];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) { r[q][0] = px[off[q] / 4]; r[q][1] = px[off[q] / 4 + 1]; }
#pragma unroll
                    for (int q = 0; q < NQ; ++q) { rb[q][0] = pb[off[q] / 4]; rb[q][1] = pb[off[q] / 4 + 1]; }
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const cf4 x0 = r[q][0], x1 = r[q][1], b0 = rb[q][0], b1 = rb[q][1];
                        const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                        const float bs[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                        for (int c = 0; c < 8; ++c) { v[q][c] = xs[c]; bv[q][c] = bs[c]; }
                    }
                } else {
                    const u32x4* px = (const u32x4*)sg.x;
                    const u32x4* pb = has_base ? (const u32x4*)sg.base : px;
                    u32x4 r[NQ], rb[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) r[q] = px[off[q] / 8];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) rb[q] = pb[off[q] / 8];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) { decode16x8(r[q], sg.dtype, v[q]); decode16x8(rb[q], sg.dtype, bv[q]); }
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    float ps = 0.f;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        float x = (v[q][c] - (has_base ? bv[q][c] : 0.f)) * sg.prescale;
                        if (!ok[q]) x = 0.f;
                        dst[q * 8 + c] = x;
                        ps += x * x;
                    }
                    ss += ps;
                }
            };
            load_signal(sgA, s.xr, sa);
            load_signal(sgB, s.xi, sb);
        } else {
#pragma unroll
            for (int q = 0; q < EMAX; ++q) {
                const int n = t + q * T;
                float va = 0.f, vb = 0.f;
                if (valid && n < C) {
                    const size_t off = (size_t)row * p.row_stride + n;
                    va = load_sig1(sgA, off);
                    vb = load_sig1(sgB, off);
                }
                s.xr[q] = va; s.xi[q] = vb;
                sa += (double)va * va; sb += (double)vb * vb;
            }
        }
        s.red[0] = sa; s.red[1] = sb;
    });
    ex.template block_sum<2>(st, [&](const double* tot) {
        partials_[2 * (size_t)pbid] = tot[0];
        partials_[2 * (size_t)pbid + 1] = tot[1];
    });

    wg_fft<P, f1_pack<P>(), 1>(ex, st, pl, lds,
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;          // natural scatter
            const int g = tid / T, t = tid % T;
            float* l = lds + g * LF;
            const float* x = comp_of<comp>(s);
            if (vec) {
#pragma unroll
                for (int q = 0; q < EMAX / 8; ++q) {
                    const int n0 = 8 * (t + q * T);
                    if (n0 < C) {
#pragma unroll
                        for (int c = 0; c < 8; ++c) l[lpad(n0 + c)] = x[q * 8 + c];
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < EMAX; ++q) {
                    const int n = t + q * T;
                    if (n < C) l[lpad(n)] = x[q];
                }
            }
        },
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;          // final gather: pairs (k, C-k)
            int tid_ = tid;
            if constexpr (f1_opaque<P>()) SM_OPAQUE(tid_);         // 128-VGPR plans: addresses recomputed here, not carried from the top
            const int g = tid_ / T, t = tid_ % T;
            const float* l = lds + g * LF;
            float* o = comp_of<comp>(s);
#pragma unroll
            for (int u = 0; u < EMAX / 2 + 1; ++u) {
                const int k = t + u * T;
                if (k < p.Cb) {
                    const int k2 = (k == 0) ? 0 : C - k;
                    const float v1 = l[lpad(k)], v2 = l[lpad(k2)];
                    if (comp == 0) { o[2 * u] = 0.5f * (v1 + v2); o[2 * u + 1] = 0.5f * (v2 - v1); }   // A.re, B.im
                    else           { o[2 * u] = 0.5f * (v1 - v2); o[2 * u + 1] = 0.5f * (v1 + v2); }   // A.im, B.re
                    // an absent second signal is EXACTLY zero (its sign class matters: sign(0) = 0);
                    // the split above would leave rounding noise of random sign there
                    if (!sgB.x) o[2 * u + 1] = 0.f;
                }
            }
        },
        [&](auto comp_c) {
            // norm_mode = reference_cpu: the torch.norm summaries of the deltas that now sit in LDS in natural order
            constexpr int comp = decltype(comp_c)::value;
            if constexpr (P::is_static) {
                if constexpr (aten_fusable(P::N, P::T)) {
                    if (p.fuse.prefix)
                        aten_fused_rows<P::N, P::T>(ex, st, p.fuse, lds, LF, fuse_where(comp), [](FftState& s) { return s.fep[comp]; });
                }
            }
        });

    ex.each(st, [&](int tid, FftState& s) {
        int tid_ = tid;
        if constexpr (f1_opaque<P>()) SM_OPAQUE(tid_);
        const int g = tid_ / T, t = tid_ % T;
        const int row = bid * p.nb + g;
        if (row >= p.R) return;
        cf4* dst = t1_ + (size_t)(row / p.ilv) * p.pitch4 * p.ilv + (row % p.ilv);
#pragma unroll
        for (int u = 0; u < EMAX / 2 + 1; ++u) {
            const int k = t + u * T;
            if (k < p.Cb) {
                cf4 v;
                v.x = s.xr[2 * u]; v.y = s.xi[2 * u]; v.z = s.xi[2 * u + 1]; v.w = s.xr[2 * u + 1];
                dst[(size_t)k * p.ilv] = v;
            }
        }
    });
}

// =====================================================================
// F1Q: forward row pass with the first radix-4 step of the COLUMN transform folded in.
//
// A long column (28672 = 7 * 2^12 rows of a Llama-3-70B MLP tensor) does not fit the engine's
// efficient regime: one 1024-thread work-group per signal, lock-step, 8-byte strided reads -
// 1.8 TB/s.  Split R = 4 * R2 (decimation in time, n = n1 * R2 + n2, k = k1 + 4 * k2):
//     X[k1 + 4 k2] = sum_{n2} W_R2^{n2 k2} * ( W_R^{n2 k1} * sum_{n1} x[n1 R2 + n2] W_4^{n1 k1} )
// The inner radix-4 butterfly over rows n2, n2 + R2, n2 + 2 R2, n2 + 3 R2 and its twiddle are
// element-wise in the bin index, so the work-group that has just transformed those four ROWS
// does them (three twiddles per work-group), and the column pass runs plain R2-point
// transforms (7168 points: 256 threads, two signals per work-group) on 4 * Cb "virtual"
// columns (k1, bin).  The spectrum planes then hold each bin column in the order
// [k1][k2] instead of k - every consumer between the transforms is order-blind inside a
// column, and the inverse column pass reads that order back (k_i1, FOLD).
// T1 here is slab-major: element (n2, k1, bin) at k1 * slab_elems + ((n2 / ilv) * pitch4 + bin) * ilv + n2 % ilv
// (the column pass then strides by one real row pitch inside a 1/4-size slab, as the plain layout does).
// =====================================================================
#ifndef SM_F1Q_QB
#define SM_F1Q_QB 1          // 16-byte loads per operand in flight per batch (register budget: 128)
#endif
#ifndef SM_F1Q_PREFETCH_B
#define SM_F1Q_PREFETCH_B 1     // issue the second operand's loads before the first exchange (measured: -2..5 %)
#endif
#ifndef SM_F1Q_PACK
#define SM_F1Q_PACK 1
#endif
template <class P> constexpr bool f1q_eligible() {
    if constexpr (P::is_static) return 4 * P::T <= 1024 && (P::N / P::T) % 2 == 0 && P::N % 8 == 0; else return false;
}

struct F1QState {
    float xr[EREG];
    float xi[EREG];
    double red[4];
    u32x4 rb[EMAX / 8], rbb[EMAX / 8];      // the second operand's raw 16-bit loads, in flight during the first exchange
};

template <class P, class Ex>
SM_HD void k_f1q(Ex& ex, const F1Params& p) {
    if constexpr (!f1q_eligible<P>()) { return; } else {
    typename Ex::template State<F1QState> st;
    ex.init(st);
    float* lds = ex.lds() + LDS_SCRATCH_FLOATS;
    const FftPlanDev& pl = p.plan;
    constexpr int T = P::T, C = P::N, LF = P::lds_floats;
    constexpr int E2 = C / T / 2;                  // bins k = t + u*T, u < E2, plus the Nyquist bin (t = 0, u = E2)
    constexpr int NJ = (E2 + 3) / 4;               // main bins per thread: u = 4*jj + g
    constexpr int NQ = EMAX / 8;
    static_assert(NJ * 8 + 4 <= EREG, "register slots");
    int sig_;
    const int bid = f1_pick_signal(p.sigs, ex.bid(), p.ilv > 1 ? p.ilv : 1, sig_);
    const int pbid = p.sigs.n > 1 ? bid : ex.bid();
    SigDesc sa = p.a, sb = p.b;
    cf4* t1_ = p.t1;
    double* partials_ = p.partials;
    if (p.sigs.n > 1) {
        sa.x = p.sigs.x[sig_]; sa.base = p.sigs.base[sig_];
        sb.x = (const char*)sa.x + p.sigs.b_off; sb.base = sa.base ? (const char*)sa.base + p.sigs.b_off : nullptr;
        t1_ = p.sigs.t1[sig_]; partials_ = p.sigs.partials[sig_];
    }
    const int unit = bid;                           // n2 (or the row-pair index m2)
    const bool live = unit < p.R2;
    const bool bits16 = sa.dtype != DT_F32 && sb.dtype != DT_F32;
    const bool has_ab = sa.base != nullptr, has_b = sb.x != nullptr, has_bb = has_b && sb.base != nullptr;
    // twiddles W_R^{n2 k1}: slot A is column element n2A, slot B n2B (they differ in row-pair mode)
    const int n2A = p.rowpair ? 2 * unit : unit, n2B = p.rowpair ? 2 * unit + 1 : unit;
    cf4* const rowp = t1_ + (size_t)(unit / p.ilv) * p.pitch4 * p.ilv + (unit % p.ilv);
    const size_t slabstride = p.slab_elems;                      // slab-major: [k1][unit][bin]

    ex.each(st, [&](int, F1QState& s) { s.red[0] = 0.0; s.red[1] = 0.0; });
    // (no fused torch.norm summaries here, unlike k_f1: this kernel is one 1024-thread work-group per CU whose transform
    //  phase is fully exposed - measured on MI355X the summaries cost it +514 us per 28672 x 8192 K = 3 launch, more than
    //  the separate summary pass they would replace (454 us); the folded shapes keep k_aten_part)

    // Register budget: a 1024-thread work-group has 128 VGPRs per thread.  The operands are
    // therefore loaded one at a time, straight into the first LDS scatter (a in the pass of the
    // real component, b in the pass of the imaginary one; b's raw loads are issued before a's
    // exchange and land during it), and the last gather of the imaginary component does the
    // cross-row butterfly and the stores bin by bin instead of parking 36 more values.
    wg_fft<P, SM_F1Q_PACK, 1>(ex, st, pl, lds,
        [&](int tid, F1QState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;          // natural scatter = operand load
            int tid_ = tid;
            SM_OPAQUE(tid_);
            const int g = tid_ / T, t = tid_ % T;
            float* l = lds + g * LF;
            const size_t rowoff = (size_t)(unit + g * p.R2) * p.row_stride;
            auto okq = [&](int q) { return live && 8 * (t + q * T) < C; };
            auto offq = [&](int q) { return okq(q) ? rowoff + 8 * (t + q * T) : (size_t)0; };
            double ss = 0.0;
            if (bits16) {
                const u32x4* pa = (const u32x4*)sa.x;
                if (comp == 0) {
                    const u32x4* pab = has_ab ? (const u32x4*)sa.base : pa;
                    u32x4 ra[NQ], rab[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) ra[q] = pa[offq(q) / 8];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) rab[q] = pab[offq(q) / 8];
#if SM_F1Q_PREFETCH_B
                    const u32x4* pb = has_b ? (const u32x4*)sb.x : pa;
                    const u32x4* pbb = has_bb ? (const u32x4*)sb.base : pa;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s.rb[q] = pb[offq(q) / 8];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s.rbb[q] = pbb[offq(q) / 8];
#endif
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        float va[8], ba[8];
                        decode16x8(ra[q], sa.dtype, va);
                        decode16x8(rab[q], sa.dtype, ba);
                        const int n0 = 8 * (t + q * T);
                        float qa = 0.f;
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            float xa = (va[c] - (has_ab ? ba[c] : 0.f)) * sa.prescale;
                            if (!okq(q)) xa = 0.f;
                            if (n0 < C) l[lpad(n0 + c)] = xa;
                            qa += xa * xa;
                        }
                        ss += qa;
                    }
                } else {
#if !SM_F1Q_PREFETCH_B
                    const u32x4* pb = has_b ? (const u32x4*)sb.x : pa;
                    const u32x4* pbb = has_bb ? (const u32x4*)sb.base : pa;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s.rb[q] = pb[offq(q) / 8];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s.rbb[q] = pbb[offq(q) / 8];
#endif
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        float vb[8], bb[8];
                        decode16x8(s.rb[q], sb.dtype, vb);
                        decode16x8(s.rbb[q], sb.dtype, bb);
                        const int n0 = 8 * (t + q * T);
                        float qb = 0.f;
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            float xb = has_b ? (vb[c] - (has_bb ? bb[c] : 0.f)) * sb.prescale : 0.f;
                            if (!okq(q)) xb = 0.f;
                            if (n0 < C) l[lpad(n0 + c)] = xb;
                            qb += xb * xb;
                        }
                        ss += qb;
                    }
                }
            } else {
                const SigDesc& sg = comp == 0 ? sa : sb;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    float v[8];
                    if (sg.x) load_sig8(sg, offq(q), v);
                    else { for (int c = 0; c < 8; ++c) v[c] = 0.f; }
                    const int n0 = 8 * (t + q * T);
                    float ps = 0.f;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const float x = okq(q) ? v[c] : 0.f;
                        if (n0 < C) l[lpad(n0 + c)] = x;
                        ps += x * x;
                    }
                    ss += ps;
                }
            }
            s.red[comp] += ss;
        },
        [&](int tid, F1QState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            // every thread takes a quarter of the bins, of ALL FOUR rows.  The real component's
            // pass parks (A.re, B.im) in xr[(jj*4 + g')*2 + {0,1}]; the imaginary component's
            // pass gets (A.im, B.re), does the radix-4 butterfly over the rows and stores.
            int tid_ = tid;
            SM_OPAQUE(tid_);                           // addresses below are recomputed here, not carried from the top
            const int g = tid_ / T, t = tid_ % T;
            auto emit = [&](int k, const float* are, const float* aim, const float* bre, const float* bim) {
                SM_SCHED_FENCE();                      // one bin's butterflies at a time (register pressure)
                float ar[4], ai[4], br[4], bi[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { ar[q] = are[q]; ai[q] = aim[q]; br[q] = has_b ? bre[q] : 0.f; bi[q] = has_b ? bim[q] : 0.f; }
                Dft<4>::run(ar, ai);
                Dft<4>::run(br, bi);
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) {
                    if (k1) {
                        // work-group-uniform addresses: the twiddles come through the scalar cache, not VGPRs
                        const cf2 wa = p.twR[(size_t)n2A * k1], wb = p.twR[(size_t)n2B * k1];
                        cmul(ar[k1], ai[k1], wa.x, wa.y); cmul(br[k1], bi[k1], wb.x, wb.y);
                    }
                    cf4 v = {ar[k1], ai[k1], br[k1], bi[k1]};
                    if (live) rowp[(size_t)k * p.ilv + k1 * slabstride] = v;
                }
                SM_SCHED_FENCE();
            };
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int u = 4 * jj + g;
                if (u < E2) {
                    const int k = t + u * T;
                    const int k2 = (k == 0) ? 0 : C - k;
                    float aim[4], bre[4];
#pragma unroll
                    for (int gp = 0; gp < 4; ++gp) {
                        const float* l = lds + gp * LF;
                        const float v1 = l[lpad(k)], v2 = l[lpad(k2)];
                        const int sl = (jj * 4 + gp) * 2;
                        if (comp == 0) { s.xr[sl] = 0.5f * (v1 + v2); s.xr[sl + 1] = 0.5f * (v2 - v1); }   // A.re, B.im
                        else           { aim[gp] = 0.5f * (v1 - v2); bre[gp] = 0.5f * (v1 + v2); }           // A.im, B.re
                    }
                    if (comp == 1) {
                        float are[4], bim[4];
#pragma unroll
                        for (int gp = 0; gp < 4; ++gp) { are[gp] = s.xr[(jj * 4 + gp) * 2]; bim[gp] = s.xr[(jj * 4 + gp) * 2 + 1]; }
                        emit(k, are, aim, bre, bim);
                    }
                }
            }
            if (tid == 0) {                                  // the Nyquist bin k = C/2: its own twin
                if (comp == 0) {
#pragma unroll
                    for (int gp = 0; gp < 4; ++gp) s.xr[NJ * 8 + gp] = lds[gp * LF + lpad(C / 2)];
                } else {
                    float are[4], aim[4] = {0.f, 0.f, 0.f, 0.f}, bre[4], bim[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int gp = 0; gp < 4; ++gp) { are[gp] = s.xr[NJ * 8 + gp]; bre[gp] = lds[gp * LF + lpad(C / 2)]; }
                    emit(C / 2, are, aim, bre, bim);
                }
            }
        });

    ex.template block_sum<2>(st, [&](const double* tot) {
        partials_[2 * (size_t)pbid] = tot[0];
        partials_[2 * (size_t)pbid + 1] = tot[1];
    });
    }
}

// =====================================================================
// F2: forward column pass (one half-spectrum bin column of A and of B)
// =====================================================================
// One launch over the slices of a rank > 2 tensor or the row blocks of a split column length: the
// grid is `wgs` work-groups per slice (0: a single slice); the slices' T1 / G and planes lie
// t1_stride (float4, or float2 for G) and plane_stride (floats) apart.
struct SliceGrid { int wgs = 0; size_t t1_stride = 0, plane_stride = 0; };
template <class Ex> SM_HD int slice_of(Ex& ex, const SliceGrid& sl, int& bid) {
    bid = ex.bid();
    if (sl.wgs <= 0) return 0;
    const int s = bid / sl.wgs;
    bid -= s * sl.wgs;
    return s;
}

struct F2Params {
    FftPlanDev plan;       // N = R
    const cf4* t1;
    int pitch4;
    int ilv;               // see F1Params
    int R, C, Cb;
    int nsig;              // 2: A and B in one work-group; 1: one signal per work-group
    int swap;              // 1: slot B plays role "a" (the larger-norm input)
    float scale[2];        // per slot: 1/norm (or the arithmetic branch's scale)
    float* reA; float* imA; float* reB;     // planes [Cb][R]; role b writes only reB
    unsigned long long* hist;               // level-1 histogram (HIST1_BINS) or null
    // FOLD variants (see k_f1q): R is the sub-length R2, Cb counts the 4 * slab virtual columns
    int slab;              // virtual columns per k1 (the real T1 pitch in float4)
    int Cb_real;           // bins per slab that exist (C/2 + 1)
    int Rfull;             // 4 * R: a bin column of the planes
    size_t slab_elems;     // float4 per k1 slab of T1 (slab-major: the row stride stays one real pitch)
    SliceGrid sl;          // several slices (rank > 2 tensor / row blocks of a split column length) in one launch
};
// virtual column v of a folded column pass -> plane offset of its first element, real bin (or -1)
SM_HD int fold_bin(int v, int slab, int Cb_real, int R2, int Rfull, size_t& off) {
    const int k1 = v / slab, k = v % slab;
    off = (size_t)k * Rfull + (size_t)k1 * R2;
    return k < Cb_real ? k : -1;
}

// BINS adjacent bin columns per work-group (2*BINS transforms, 2*BINS*T threads): the
// row segment a work-group reads is BINS*16 bytes wide, so short columns get full
// 128-byte segments (BINS = 8) and 8192-long ones 32 bytes.
// Layout and grouping rules shared with the host (sm_pipeline.hpp: t1_interleave(), run_f2()).
// For a static plan the column length is known, so both are compile-time constants and the
// kernel contains one variant only (the union of all variants cost ~10 % through register
// allocation alone).
#ifndef SM_T1_ILV
#define SM_T1_ILV 2
#endif
#ifndef SM_T1_ILV_MIN_ROWS
#define SM_T1_ILV_MIN_ROWS 8192
#endif
#ifndef SM_F2_MAX_THREADS
#define SM_F2_MAX_THREADS 512
#endif
SM_HD constexpr int t1_interleave_rows(int R) { return R >= SM_T1_ILV_MIN_ROWS ? SM_T1_ILV : 1; }
SM_HD constexpr int f2_nsig_for(int T) { return (2 * T <= SM_F2_MAX_THREADS) ? 2 : 1; }

constexpr int FOLD_ILV = 2;      // rows n2, n2 + 1 interleaved in T1 on the folded path: 32-byte pieces
template <class P> constexpr bool fold_col_plan() {          // lengths used as R2 = R / 4
    if constexpr (P::is_static) return f2_nsig_for(P::T) == 2 && (P::N == 2048 || P::N == 3584 || P::N == 4096 || P::N == 7168);
    else return false;
}
template <class P, int BINS, bool FOLD = false, class Ex>
SM_HD void k_f2(Ex& ex, const F2Params& p) {
    if constexpr (FOLD && !fold_col_plan<P>()) { return; } else {
    typename Ex::template State<FftState> st;
    ex.init(st);
    float* lds = ex.lds() + LDS_SCRATCH_FLOATS;
    const FftPlanDev& pl = p.plan;
    const int T = plan_T<P>(pl), R = plan_N<P>(pl);
    const int LF = plan_lds<P>(pl);
    const int ng = P::is_static ? f2_nsig_for(T) : p.nsig;              // compile-time for static plans
    const int ilv = FOLD ? FOLD_ILV : (P::is_static ? t1_interleave_rows(R) : p.ilv);
    int bid;
    const int slice = slice_of(ex, p.sl, bid);
    const cf4* const t1 = p.t1 + slice * p.sl.t1_stride;
    const size_t pl_off = slice * p.sl.plane_stride;
    // 8/BINS work-groups share a 128-byte line of T1 (16 bytes per bin)
    // (one signal per work-group, T = 1024: the 16 work-groups of a line - 8 bins x 2 signals)
    const int lbid = (ng == 2) ? xcd_remap(bid, 8 / BINS) : xcd_remap(bid, 16);
    const int kbase = (ng == 2) ? lbid * BINS : lbid / 2;
    const int slot0 = (ng == 2) ? 0 : lbid % 2;
    if (kbase >= p.Cb) return;
    const int ngroups = (ng == 2) ? 2 * BINS : 1;
    const int nthreads = ngroups * T;
    uint32_t* lhist = (uint32_t*)(lds + ngroups * LF);

    ex.each(st, [&](int tid, FftState& s) {
        if (ng == 2) {
            const int b = tid % BINS, lane = tid / BINS;
            const int k2 = kbase + b;
            // slot q holds row f2_row(lane, q): ILV consecutive rows of a thread are one
            // contiguous ILV*16-byte piece of T1
            auto load_rows = [&](auto ilv_c) {
                constexpr int ILV = decltype(ilv_c)::value;
#pragma unroll
                for (int q = 0; q < EMAX / 2; ++q) {
                    const int m = lane + (q / ILV) * 2 * T;               // row group
                    const int n = m * ILV + q % ILV;
                    // (clamped address, masked value: see k_f2s)
                    const bool live = n < R && k2 < p.Cb;
                    const int kc = k2 < p.Cb ? k2 : p.Cb - 1;
                    const int mcl = n < R ? m : (R - 1 - q % ILV) / ILV;
                    cf4 v;
                    if constexpr (FOLD) {
                        // slab-major T1: virtual column k2 = (k1, bin) lives in slab k1, row pitch = slab
                        v = t1[(size_t)(kc / p.slab) * p.slab_elems + ((size_t)mcl * p.slab + (kc % p.slab)) * ILV + q % ILV];
                    } else {
                        v = t1[((size_t)mcl * p.pitch4 + kc) * ILV + q % ILV];
                    }
                    s.xr[2 * q] = live ? v.x : 0.f; s.xi[2 * q] = live ? v.y : 0.f; s.xr[2 * q + 1] = live ? v.z : 0.f; s.xi[2 * q + 1] = live ? v.w : 0.f;
                }
            };
            if (ilv == 2) load_rows(std::integral_constant<int, 2>{});
            else load_rows(std::integral_constant<int, 1>{});
        } else {
#pragma unroll
            for (int q = 0; q < EMAX; ++q) {
                const int n = tid + q * T;
                float re = 0.f, im = 0.f;
                if (n < R) {
                    const cf2* src = (const cf2*)(t1 + ((size_t)(n / ilv) * p.pitch4 + kbase) * ilv + n % ilv) + slot0;
                    re = src->x; im = src->y;
                }
                s.xr[q] = re; s.xi[q] = im;
            }
        }
        if (p.hist) for (int h = tid; h < HIST1_BINS; h += nthreads) lhist[h] = 0;
    });

#ifndef SM_F2_PACK
#define SM_F2_PACK 1
#endif
    wg_fft<P, SM_F2_PACK, 2>(ex, st, pl, lds,
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            const float* x = comp_of<comp>(s);
            if (ng == 2) {
                const int b = tid % BINS, lane = tid / BINS;
                float* la = lds + (2 * b) * LF;
                auto scatter_rows = [&](auto ilv_c) {
                    constexpr int ILV = decltype(ilv_c)::value;
#pragma unroll
                    for (int q = 0; q < EMAX / 2; ++q) {
                        const int n = (lane + (q / ILV) * 2 * T) * ILV + q % ILV;
                        if (n < R) { la[lpad(n)] = x[2 * q]; la[LF + lpad(n)] = x[2 * q + 1]; }
                    }
                };
                if (ilv == 2) scatter_rows(std::integral_constant<int, 2>{});
                else scatter_rows(std::integral_constant<int, 1>{});
            } else {
#pragma unroll
                for (int q = 0; q < EMAX; ++q) {
                    const int n = tid + q * T;
                    if (n < R) lds[lpad(n)] = x[q];
                }
            }
        },
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            const int g = tid / T, t = tid % T;
            const float* l = lds + g * LF;
            float* o = comp_of<comp>(s);
#pragma unroll
            for (int u = 0; u < EMAX / 4; ++u) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k1 = 4 * (t + u * T) + c;
                    if (k1 < R) o[4 * u + c] = l[lpad(k1)];
                }
            }
        });

    ex.each(st, [&](int tid, FftState& s) {
        const int g = tid / T, t = tid % T;
        const int slot = (ng == 2) ? (g & 1) : slot0;
        const int k2 = kbase + ((ng == 2) ? (g >> 1) : 0);
        if (k2 >= p.Cb) return;
        const bool role_a = (slot ^ p.swap) == 0;
        const float sc = p.scale[slot];
        size_t poff = (size_t)k2 * R;
        int kreal = k2;
        if constexpr (FOLD) { kreal = fold_bin(k2, p.slab, p.Cb_real, R, p.Rfull, poff); if (kreal < 0) return; }
        const uint32_t w = (uint32_t)bin_weight(kreal, p.C);
        float* dre = (role_a ? p.reA : p.reB) + pl_off + poff;
        float* dim = p.imA + pl_off + poff;
#pragma unroll
        for (int u = 0; u < EMAX / 4; ++u) {
            const int k0 = 4 * (t + u * T);
            if (k0 + 3 < R && (R & 3) == 0) {
                cf4 vr = {s.xr[4 * u] * sc, s.xr[4 * u + 1] * sc, s.xr[4 * u + 2] * sc, s.xr[4 * u + 3] * sc};
                *(cf4*)(dre + k0) = vr;
                if (role_a) {
                    cf4 vi = {s.xi[4 * u] * sc, s.xi[4 * u + 1] * sc, s.xi[4 * u + 2] * sc, s.xi[4 * u + 3] * sc};
                    *(cf4*)(dim + k0) = vi;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (k0 + c < R) {
                        dre[k0 + c] = s.xr[4 * u + c] * sc;
                        if (role_a) dim[k0 + c] = s.xi[4 * u + c] * sc;
                    }
                }
            }
            if (p.hist) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (k0 + c < R) {
                        const uint32_t key = f2u(s.xr[4 * u + c] * sc) & 0x7fffffffu;
                        ex.lds_atomic_add(&lhist[key >> 20], w);
                    }
                }
            }
        }
    });
    if (p.hist) {
        ex.sync();
        ex.each(st, [&](int tid, FftState&) {
            for (int h = tid; h < HIST1_BINS; h += nthreads) {
                const uint32_t v = lhist[h];
                if (v) ex.global_atomic_add(&p.hist[h], (unsigned long long)v);
            }
        });
    }
    }
}

// bins per work-group of the column passes for a plan with T threads per transform
// (measured on MI355X: 1024-thread work-groups lose more than their wider row segments
//  gain - 8192^2: F2 382 -> 415 us, I1 164 -> 203 us - so the target is 512 threads)
#ifndef SM_COL_THREADS
#define SM_COL_THREADS 512
#endif
// (the 256-point row blocks of a split column length are so short that a work-group's fixed
//  costs - its histogram flush above all: the same ~150 hot addresses from every work-group - outweigh
//  its payload: 8 bins there, whole 128-byte lines of T1, half the work-groups)
constexpr int f2_bins_for(int T, int N = 1 << 30) {
    if (T == 64 && N <= 256) return 8;        // (measured: 512-point blocks lose 20 % with 8)
    return (SM_COL_THREADS / (2 * T)) > 1 ? (SM_COL_THREADS / (2 * T) > 8 ? 8 : SM_COL_THREADS / (2 * T)) : 1;
}
// the inverse column pass measured fastest with two bins per work-group at every length
#ifndef SM_I1_THREADS
constexpr int i1_bins_for(int T) { return 2; }     // the host launches KI1x1 instead when 2T is too large
#else
constexpr int i1_bins_for(int T) { return (SM_I1_THREADS / T) > 2 ? ((SM_I1_THREADS / T) > 16 ? 16 : (SM_I1_THREADS / T)) : 2; }
#endif
template <class P> constexpr int f2_bins() { if constexpr (P::is_static) return f2_bins_for(P::T, P::N); else return 1; }
template <class P> constexpr int i1_bins() { if constexpr (P::is_static) return i1_bins_for(P::T); else return 2; }

// ---------------------------------------------------------------------------------
// F2S: forward column pass of ONE signal (tournament rounds >= 2: the other input of the pair is
// an intermediate that stayed in the spectral domain).  The row pass ran in row-pair mode
// (F1Params::row_stride = 2C): T1[m][k] = (row 2m's bin k, row 2m+1's bin k), so one float4 holds
// two CONSECUTIVE elements of a column.  A work-group transforms G adjacent bin columns
// (G = the 2*BINS transforms of the two-signal kernel, same threads / LDS), reading G*16
// contiguous bytes per row pair.  role_a: the signal is the pair's larger-norm input (writes
// Re a, Im a), else it writes Re b only.
// ---------------------------------------------------------------------------------
struct F2SParams {
    FftPlanDev plan;       // N = R (even)
    const cf4* t1;         // [R/2][pitch4]
    int pitch4;
    int R, C, Cb;
    int role_a;
    float scale;
    float* re; float* im;  // destination planes [Cb][R] (im unused when !role_a)
    unsigned long long* hist;
    int slab, Cb_real, Rfull;   // FOLD variant: as F2Params
    size_t slab_elems;
    double* im_partials;        // role a only, or null: [grid] sum w (Im a)^2 of what this work-group stored
                                // (the Parseval norm of the pair's result when it stays spectral)
    SliceGrid sl;
    // two = 1: BOTH inputs of a pair in one launch (one role a, one role b; no slices): the second signal's T1, role,
    // scale and Re plane; the work-groups of the two signals alternate in blocks of XG (pick_signal) - one launch
    // boundary less per pair merge
    int two;
    const cf4* t1_2; int role_a_2; float scale_2; float* re_2;
};
template <class P> constexpr int f2s_groups() {
    if constexpr (P::is_static) return f2_nsig_for(P::T) == 2 ? 2 * f2_bins_for(P::T, P::N) : 1; else return 1;
}

#ifndef SM_F2S_ILV
#define SM_F2S_ILV 1        // 2 = row PAIRS interleaved in the single-signal T1 (64-byte pieces for the column pass): measured on
                            // MI355X it takes 4-12 % off f2s and puts 8-12 % on the row pass (half-line stores) - net loss
#endif
constexpr int F2S_ILV = SM_F2S_ILV;
// DIRECT (round 4): the column pass takes its loads straight into the first radix pass's layout and stores straight out
// of the last one's - two of the transform's four exchanges through LDS (and 8 of its 16 barriers) go away:
//  * first pass, butterfly j = t + m T takes rows j + i N/R0: lanes 2k and 2k + 1 need the SAME row pairs (T1 holds rows
//    2m, 2m + 1 in one float4) - the even lane loads the pairs of even i, the odd lane those of odd i, and they trade
//    halves through a quad-permute DPP move (Ex::lane_pair_trade), no LDS;
//  * last pass, thread t holds outputs t + T u: 64 lanes store 256 contiguous bytes per instruction (dword stores;
//    measured with tools/membench2.hip: as fast as the exchanged 16-byte form at two columns per work-group).
// Columns are dealt by thread group (g = tid / T) instead of by lane (tid % G): the loader must be the owner.
// MEASURED ON MI355X AND LEFT OFF (profiles/r04_ab_f2s_direct.txt): bit-identical results, but the owner-loads mapping
// gives up the 32-byte pieces two adjacent lanes read (f2s 529 -> 583 us at 28672 x 8192, 464 -> 567 at 8192 x 28672)
// and the dword stores lose more than the exchange they save on the 8192-point plan (464 -> 531; 529 -> 516 on the
// folded 7168-point one): the column passes are bound by their access pattern, not by their exchanges.
#ifndef SM_F2S_DIRECT
#define SM_F2S_DIRECT 0     // bit 0: loads into the first pass's layout (DPP trade), bit 1: stores out of the last pass's
#endif
template <class P, int G> constexpr int f2s_direct() {
    if constexpr (!P::is_static) return 0;
    else {
        constexpr int R0 = P::radix(0);
        constexpr bool ok = F2S_ILV == 1 && (G == 1 || G == 2) && P::npass >= 2 && P::T % 2 == 0 && R0 % 2 == 0 &&
                            (P::N / R0) % 2 == 0 && (EMAX / R0) * R0 * P::T >= P::N;
        return ok ? (SM_F2S_DIRECT & 3) : 0;
    }
}
template <class P, int G, bool FOLD = false, class Ex>
SM_HD void k_f2s(Ex& ex, const F2SParams& p) {
    if constexpr (FOLD && !fold_col_plan<P>()) { return; } else {
    typename Ex::template State<FftState> st;
    ex.init(st);
    float* lds = ex.lds() + LDS_SCRATCH_FLOATS;
    const FftPlanDev& pl = p.plan;
    const int T = plan_T<P>(pl), R = plan_N<P>(pl);
    const int LF = plan_lds<P>(pl);
    constexpr int XG = G >= 8 ? 1 : 8 / G;                 // work-groups that share a 128-byte line of T1
    int bid_in_slice;
    const int slice = slice_of(ex, p.sl, bid_in_slice);
    int sig2 = 0;
    const int lbid = p.two ? pick_signal(2, bid_in_slice, XG, sig2) : xcd_remap(bid_in_slice, XG);
    const cf4* const t1 = (sig2 ? p.t1_2 : p.t1) + slice * p.sl.t1_stride;
    const size_t pl_off = slice * p.sl.plane_stride;
    const int role_a_ = sig2 ? p.role_a_2 : p.role_a;
    const float scale_ = sig2 ? p.scale_2 : p.scale;
    float* const re_ = sig2 ? p.re_2 : p.re;
    const int kbase = lbid * G;
    if (kbase >= p.Cb) {                      // padding work-group: its partial must still read zero
        if (p.im_partials) ex.each(st, [&](int tid, FftState&) { if (tid == 0) p.im_partials[ex.bid()] = 0.0; });
        return;
    }
    const int nthreads = G * T;
    const int half = R / 2;
    uint32_t* lhist = (uint32_t*)(lds + G * LF);

    constexpr int DIRECT = f2s_direct<P, G>();
    if constexpr ((DIRECT & 1) != 0) {
        constexpr int R0 = P::radix(0), MB0 = EMAX / R0, nb0 = P::N / R0;
        ex.each(st, [&](int tid, FftState& s) {
            const int g = tid / T, t = tid % T;
            const int k2 = kbase + g;
            const int kc = k2 < p.Cb ? k2 : p.Cb - 1;
            const int par = t & 1;
            // (clamped address, masked value: a load behind a branch is waited for on the spot)
            static_for<0, MB0>([&](auto m_c) {
                constexpr int m = decltype(m_c)::value;
                const bool live = (t + m * T) < nb0 && k2 < p.Cb;
                static_for<0, R0 / 2>([&](auto q_c) {
                    constexpr int q = decltype(q_c)::value;
                    // the row pair of rows j + i nb0, j = t + m T, i = 2 q + par (nb0, T even)
                    const int pm = live ? (t >> 1) + m * (T / 2) + q * nb0 + par * (nb0 / 2) : 0;
                    cf4 v;
#if defined(SM_DIAG_NOMEM)
                    v = cf4{(float)q, (float)t, 1.f, (float)kc};
#else
                    if constexpr (FOLD) v = t1[(size_t)(kc / p.slab) * p.slab_elems + (size_t)pm * p.slab + (kc % p.slab)];
                    else v = t1[(size_t)pm * p.pitch4 + kc];
#endif
                    s.xr[m * R0 + 2 * q] = live ? v.x : 0.f; s.xi[m * R0 + 2 * q] = live ? v.y : 0.f;
                    s.xr[m * R0 + 2 * q + 1] = live ? v.z : 0.f; s.xi[m * R0 + 2 * q + 1] = live ? v.w : 0.f;
                });
            });
            if (p.hist) for (int h = tid; h < HIST1_BINS; h += nthreads) lhist[h] = 0;
        });
        // the even lane holds (own rows of i = 2q | the partner's rows of i = 2q), the odd lane the mirror image
        ex.template lane_pair_trade<MB0 * (R0 / 2) * 2>(st, [](FftState& s, auto k_c) {
            constexpr int k = decltype(k_c)::value;
            constexpr int idx = k / 2, m = idx / (R0 / 2), q = idx % (R0 / 2);
            float* arr = (k % 2) ? s.xi : s.xr;
            return FloatPairRef{arr[m * R0 + 2 * q], arr[m * R0 + 2 * q + 1]};
        });
    } else
    ex.each(st, [&](int tid, FftState& s) {
        const int b = tid % G, lane = tid / G;
        const int k2 = kbase + b;
#pragma unroll
        for (int q = 0; q < EMAX / 2; ++q) {
            const int m = F2S_ILV * (lane + (q / F2S_ILV) * T) + q % F2S_ILV;      // row pair (rows 2m, 2m+1)
            // (the address is clamped, the value masked afterwards: behind a branch every load is waited for on the
            // spot - the 7168-point plan, whose last two slots are empty, ran its 14 strided loads one after the other)
            const bool live = m < half && k2 < p.Cb;
            const int mc = m < half ? m : half - 1, kc = k2 < p.Cb ? k2 : p.Cb - 1;
            cf4 v;
#if defined(SM_DIAG_NOMEM)
            v = cf4{(float)q, (float)lane, 1.f, (float)kc};          // diagnostic build: no global loads
#else
            if constexpr (FOLD) {
                v = t1[(size_t)(kc / p.slab) * p.slab_elems + ((size_t)(mc / F2S_ILV) * p.slab + (kc % p.slab)) * F2S_ILV + mc % F2S_ILV];
            } else {
                v = t1[((size_t)(mc / F2S_ILV) * p.pitch4 + kc) * F2S_ILV + mc % F2S_ILV];
            }
#endif
            s.xr[2 * q] = live ? v.x : 0.f; s.xi[2 * q] = live ? v.y : 0.f; s.xr[2 * q + 1] = live ? v.z : 0.f; s.xi[2 * q + 1] = live ? v.w : 0.f;
        }
        if (p.hist) for (int h = tid; h < HIST1_BINS; h += nthreads) lhist[h] = 0;
    });

#ifndef SM_F2S_PACK
#define SM_F2S_PACK 1
#endif
    wg_fft<P, SM_F2S_PACK, 4, DIRECT>(ex, st, pl, lds,
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            const float* x = comp_of<comp>(s);
            const int b = tid % G, lane = tid / G;
            float* la = lds + b * LF;
#pragma unroll
            for (int q = 0; q < EMAX / 2; ++q) {
                const int m = F2S_ILV * (lane + (q / F2S_ILV) * T) + q % F2S_ILV;
                if (m < half) { la[lpad(2 * m)] = x[2 * q]; la[lpad(2 * m + 1)] = x[2 * q + 1]; }
            }
        },
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            const int g = tid / T, t = tid % T;
            const float* l = lds + g * LF;
            float* o = comp_of<comp>(s);
#pragma unroll
            for (int u = 0; u < EMAX / 4; ++u) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k1 = 4 * (t + u * T) + c;
                    if (k1 < R) o[4 * u + c] = l[lpad(k1)];
                }
            }
        });

    ex.each(st, [&](int tid, FftState& s) {
        const int g = tid / T, t = tid % T;
        const int k2 = kbase + g;
        s.red[0] = 0.0;
        if (k2 >= p.Cb) return;
        const float sc = scale_;
        size_t poff = (size_t)k2 * R;
        int kreal = k2;
        if constexpr (FOLD) { kreal = fold_bin(k2, p.slab, p.Cb_real, R, p.Rfull, poff); if (kreal < 0) return; }
        const uint32_t w = (uint32_t)bin_weight(kreal, p.C);
        float* dre = re_ + pl_off + poff;
        float* dim = p.im + pl_off + poff;
        float imsq = 0.f;
        if constexpr ((DIRECT & 2) != 0) {
            // last-pass layout: slot m RL + i is output j + i NsL, j = t + m T: consecutive lanes, consecutive floats
            constexpr int RL = P::radix(P::npass - 1), MBL = EMAX / RL, NsL = P::N / RL;
            static_for<0, MBL>([&](auto m_c) {
                constexpr int m = decltype(m_c)::value;
                const int j = t + m * T;
                if (j < NsL) {
                    static_for<0, RL>([&](auto i_c) {
                        constexpr int i = decltype(i_c)::value, e = m * RL + i;
                        const float vr = s.xr[e] * sc;
#if defined(SM_DIAG_NOMEM)
                        if (vr == 12345.678f)
#endif
                        dre[j + i * NsL] = vr;
                        if (role_a_) {
                            const float vi = s.xi[e] * sc;
#if defined(SM_DIAG_NOMEM)
                            if (vi == 12345.678f)
#endif
                            dim[j + i * NsL] = vi;
                            imsq += vi * vi;
                        }
                        if (p.hist) ex.lds_atomic_add(&lhist[(f2u(vr) & 0x7fffffffu) >> 20], w);
                    });
                }
            });
        } else
#pragma unroll
        for (int u = 0; u < EMAX / 4; ++u) {
            const int k0 = 4 * (t + u * T);
            if (k0 + 3 < R && (R & 3) == 0) {
                cf4 vr = {s.xr[4 * u] * sc, s.xr[4 * u + 1] * sc, s.xr[4 * u + 2] * sc, s.xr[4 * u + 3] * sc};
#if defined(SM_DIAG_NOMEM)
                if (vr.x == 12345.678f)                                  // diagnostic build: no global stores
#endif
                *(cf4*)(dre + k0) = vr;
                if (role_a_) {
                    cf4 vi = {s.xi[4 * u] * sc, s.xi[4 * u + 1] * sc, s.xi[4 * u + 2] * sc, s.xi[4 * u + 3] * sc};
#if defined(SM_DIAG_NOMEM)
                    if (vi.x == 12345.678f)
#endif
                    *(cf4*)(dim + k0) = vi;
                    imsq += vi.x * vi.x + vi.y * vi.y + vi.z * vi.z + vi.w * vi.w;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (k0 + c < R) {
                        dre[k0 + c] = s.xr[4 * u + c] * sc;
                        if (role_a_) { const float vi = s.xi[4 * u + c] * sc; dim[k0 + c] = vi; imsq += vi * vi; }
                    }
                }
            }
            if (p.hist) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (k0 + c < R) {
                        const uint32_t key = f2u(s.xr[4 * u + c] * sc) & 0x7fffffffu;
                        ex.lds_atomic_add(&lhist[key >> 20], w);
                    }
                }
            }
        }
        s.red[0] = (double)imsq * (double)w;
    });
    if (p.hist) {
        ex.sync();
        ex.each(st, [&](int tid, FftState&) {
            for (int h = tid; h < HIST1_BINS; h += nthreads) {
                const uint32_t v = lhist[h];
                if (v) ex.global_atomic_add(&p.hist[h], (unsigned long long)v);
            }
        });
    }
    if (p.im_partials) {
        ex.sync();
        ex.template block_sum<1>(st, [&](const double* tot) { p.im_partials[ex.bid()] = tot[0]; });
    }
    }
}

// R == 1 (1-D tensors): the column transform is the identity, so the column passes are
// plain element-wise kernels (a 2049-work-group launch of the transform kernel for a
// 4096-element layernorm weight cost 230 us)
template <class Ex>
SM_HD void k_f2_r1(Ex& ex, const F2Params& p) {
    typename Ex::template State<EmptyStateF> st;
    ex.init(st);
    uint32_t* lhist = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int nt = ex.nthreads();
    if (p.hist) {
        ex.each(st, [&](int tid, EmptyStateF&) { for (int h = tid; h < HIST1_BINS; h += nt) lhist[h] = 0; });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyStateF&) {
        for (int k2 = ex.bid() * nt + tid; k2 < p.Cb; k2 += ex.nblocks() * nt) {
            const cf4 v = p.t1[k2];
            const float in[2][2] = {{v.x, v.y}, {v.z, v.w}};
            const uint32_t w = (uint32_t)bin_weight(k2, p.C);
#pragma unroll
            for (int slot = 0; slot < 2; ++slot) {
                const bool role_a = (slot ^ p.swap) == 0;
                const float re = in[slot][0] * p.scale[slot], im = in[slot][1] * p.scale[slot];
                if (role_a) { p.reA[k2] = re; p.imA[k2] = im; } else { p.reB[k2] = re; }
                if (p.hist) ex.lds_atomic_add(&lhist[(f2u(re) & 0x7fffffffu) >> 20], w);
            }
        }
    });
    if (p.hist) {
        ex.sync();
        ex.each(st, [&](int tid, EmptyStateF&) {
            for (int h = tid; h < HIST1_BINS; h += nt) {
                const uint32_t v = lhist[h];
                if (v) ex.global_atomic_add(&p.hist[h], (unsigned long long)v);
            }
        });
    }
}

// =====================================================================
// I1: inverse column pass
// =====================================================================
struct I1Params {
    FftPlanDev plan;       // N = R
    const float* reR;      // Re R plane [Cb][R] (cull applied on read)
    const float* imA;      // Im plane
    const float* cull_thr; // device scalar or null: |re| < *cull_thr -> 0
    float cull_val;        // used when cull_thr is null (0: no cull)
    int R, Cb;
    int s;                 // bin columns per work-group
    cf2* G;                // [R][pitchG]
    int pitchG;
    SliceGrid sl;          // (t1_stride counts float2 of G here)
};

// FOLD: the planes hold each bin column in the folded order [k1][k2] (k = k1 + 4 k2, see k_f1q):
// the loads stay contiguous (16 bytes from slab k1), the natural position is restored in the
// first LDS scatter.
template <class P> constexpr bool fold_full_plan() {
    if constexpr (P::is_static) return P::N == 8192 || P::N == 14336 || P::N == 16384 || P::N == 28672; else return false;
}
template <class P, int S, bool FOLD = false, class Ex>
SM_HD void k_i1(Ex& ex, const I1Params& p) {
    if constexpr (FOLD && !fold_full_plan<P>()) { return; } else {
    typename Ex::template State<FftState> st;
    ex.init(st);
    float* lds = ex.lds() + LDS_SCRATCH_FLOATS;
    const FftPlanDev& pl = p.plan;
    const int T = plan_T<P>(pl), R = plan_N<P>(pl);
    const int LF = plan_lds<P>(pl);
    int bid_in_slice;
    const int slice = slice_of(ex, p.sl, bid_in_slice);
    const size_t pl_off = slice * p.sl.plane_stride;
    cf2* const Gs = p.G + slice * p.sl.t1_stride;
    const int bid = xcd_remap(bid_in_slice, 16 / S);      // 16 bins of 8 B share a 128-B line
    if (bid * S >= p.Cb) return;
    const float thr = p.cull_thr ? *p.cull_thr : p.cull_val;

    ex.each(st, [&](int tid, FftState& s) {
        const int g = tid / T, t = tid % T;
        const int k2 = bid * S + g;
        const bool valid = k2 < p.Cb;
        const float* sre = p.reR + pl_off + (size_t)k2 * R;
        const float* sim = p.imA + pl_off + (size_t)k2 * R;
#pragma unroll
        for (int u = 0; u < EMAX / 4; ++u) {
            const int k0 = 4 * (t + u * T);            // FOLD: four consecutive elements of one slab
            float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
            if (valid) {
                if (k0 + 3 < R && (R & 3) == 0) {
                    const cf4 a = *(const cf4*)(sre + k0), b = *(const cf4*)(sim + k0);
                    re[0] = a.x; re[1] = a.y; re[2] = a.z; re[3] = a.w;
                    im[0] = b.x; im[1] = b.y; im[2] = b.z; im[3] = b.w;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (k0 + c < R) { re[c] = sre[k0 + c]; im[c] = sim[k0 + c]; }
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (fabsf(re[c]) < thr) re[c] = 0.f;
                // inverse via the swap trick: ifft(x) = swap(fft(swap(x)))
                s.xr[4 * u + c] = im[c];
                s.xi[4 * u + c] = re[c];
            }
        }
    });

#ifndef SM_I1_PACK
#define SM_I1_PACK 0
#endif
    wg_fft<P, SM_I1_PACK, 8>(ex, st, pl, lds,
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            const int g = tid / T, t = tid % T;
            float* l = lds + g * LF;
            const float* x = comp_of<comp>(s);
#pragma unroll
            for (int u = 0; u < EMAX / 4; ++u) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k1 = 4 * (t + u * T) + c;
                    if (k1 < R) {
                        if constexpr (FOLD) {
                            const int R2 = R / 4;                      // stored position k1 = slab * R2 + k2
                            l[lpad((k1 / R2) + 4 * (k1 % R2))] = x[4 * u + c];
                        } else {
                            l[lpad(k1)] = x[4 * u + c];
                        }
                    }
                }
            }
        },
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            float* o = comp_of<comp>(s);
            // thread handles the row PAIRS m = tid + j*(S*T) (rows 2m, 2m+1) and needs every
            // group's value: slot (2j + par)*S + g
#pragma unroll
            for (int j = 0; j < EMAX / (2 * S); ++j) {
                const int m = tid + j * S * T;
#pragma unroll
                for (int par = 0; par < 2; ++par) {
                    const int r = 2 * m + par;
                    if (r < R) {
#pragma unroll
                        for (int g = 0; g < S; ++g) o[(2 * j + par) * S + g] = lds[g * LF + lpad(r)];
                    }
                }
            }
        });

    // G is stored in row pairs, [R/2][pitchG][2] float2: the inverse row pass takes rows
    // (2m, 2m+1) as one complex transform, and this pass writes 16 contiguous bytes per
    // (pair, bin) - 32 with two bins - whatever the number of bins per work-group
    ex.each(st, [&](int tid, FftState& s) {
#pragma unroll
        for (int j = 0; j < EMAX / (2 * S); ++j) {
            const int m = tid + j * S * T;
            if (2 * m < R) {
                cf4* dst = (cf4*)Gs + (size_t)m * p.pitchG + (size_t)bid * S;
                const bool odd = 2 * m + 1 < R;
#pragma unroll
                for (int g = 0; g < S; ++g) {
                    if (bid * S + g < p.pitchG) {
                        // swap trick: true (re, im) = (xi, xr)
                        const int e0 = (2 * j) * S + g, e1 = (2 * j + 1) * S + g;
                        cf4 v = {s.xi[e0], s.xr[e0], odd ? s.xi[e1] : 0.f, odd ? s.xr[e1] : 0.f};
                        dst[g] = v;
                    }
                }
            }
        }
    });
    }
}

template <class Ex>
SM_HD void k_i1_r1(Ex& ex, const I1Params& p) {
    typename Ex::template State<EmptyStateF> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const float thr = p.cull_thr ? *p.cull_thr : p.cull_val;
    ex.each(st, [&](int tid, EmptyStateF&) {
        for (int k2 = ex.bid() * nt + tid; k2 < p.Cb; k2 += ex.nblocks() * nt) {
            float re = p.reR[k2];
            if (fabsf(re) < thr) re = 0.f;
            cf4 v = {re, p.imA[k2], 0.f, 0.f};           // row pair (0, -)
            ((cf4*)p.G)[k2] = v;
        }
    });
}

// =====================================================================
// I2: inverse row pass, two rows per transform
// =====================================================================
struct I2Params {
    FftPlanDev plan;       // N = C
    const cf2* G;
    int pitchG;
    int R, C, Cb;
    int nb;                // row pairs per work-group
    int vec;               // C % 8 == 0 (and aligned out/base)
    float inv_n;           // 1/(R*C): the inverse transform's normalisation
    float post;            // target_norm (1 for the arithmetic branch / raw merges)
    int ifft_policy;       // 1: NaN -> 0 (counted) and Inf flagged right after the inverse transform
    const void* base; int base_dtype;   // add-back tensor or null
    void* out; int out_mode;
    uint32_t* flags;       // [0] NaNs zeroed after ifft, [1] Inf after ifft, [2] NaNs zeroed after add-back, [3] Inf after add-back
    double* norm_partials; // [grid][2] or null: sum of squares of what this work-group stored (next round's ||merged||)
};

SM_HD void i2_finish(const I2Params& p, float v, size_t off, uint32_t& nan1, uint32_t& inf1, uint32_t& nan2, uint32_t& inf2, float& outv) {
    v *= p.inv_n;
    if (p.ifft_policy) {
        if (is_nan(v)) { v = 0.f; nan1++; }
        if (is_inf(v)) inf1 = 1;
    }
    v *= p.post;
    if (p.base) {
        v += load_elem(p.base, p.base_dtype, off);
        if (is_nan(v)) { v = 0.f; nan2++; }
        if (is_inf(v)) inf2 = 1;
    }
    outv = v;
}

template <class P, class Ex>
SM_HD void k_i2(Ex& ex, const I2Params& p) {
    typename Ex::template State<FftState> st;
    ex.init(st);
    float* lds = ex.lds() + LDS_SCRATCH_FLOATS;
    const FftPlanDev& pl = p.plan;
    const int T = plan_T<P>(pl), C = plan_N<P>(pl);
    const int LF = plan_lds<P>(pl);
    const int bid = ex.bid();
    const bool vec = P::is_static ? true : (p.vec != 0);      // see k_f1

    ex.each(st, [&](int tid, FftState& s) {
        const int g = tid / T, t = tid % T;
        const int r0 = 2 * (bid * p.nb + g), r1 = r0 + 1;
        const bool v0 = r0 < p.R, v1 = r1 < p.R;
        // loads are issued in two batches, none inside a divergent branch (out-of-range
        // ones are clamped to a valid address and masked), so each batch is in flight together
        const cf4* GP = (const cf4*)p.G + (size_t)(v0 ? r0 / 2 : 0) * p.pitchG;     // row pairs, see k_i1
        constexpr int NU = EMAX / 2 + 1, HU = (NU + 1) / 2;
        static_for<0, 2>([&](auto half_c) {
            constexpr int u0 = decltype(half_c)::value * HU;
            constexpr int u1 = (u0 + HU < NU) ? u0 + HU : NU;
            cf4 ap[HU];
#pragma unroll
            for (int u = u0; u < u1; ++u) {
                const int k = t + u * T;
                ap[u - u0] = GP[k < p.Cb ? k : 0];
            }
#pragma unroll
            for (int u = u0; u < u1; ++u) {
                const int k = t + u * T;
                if (k < p.Cb) {
                    cf2 g0 = {ap[u - u0].x, ap[u - u0].y}, g1 = {ap[u - u0].z, ap[u - u0].w};
                    if (!v0) { g0.x = 0.f; g0.y = 0.f; }
                    if (!v1) { g1.x = 0.f; g1.y = 0.f; }
                    if (k == 0 || 2 * k == C) { g0.y = 0.f; g1.y = 0.f; }   // c2r: DC / Nyquist are real
                    // Y[k] = G0[k] + i G1[k];  Y[C-k] = conj(G0[k]) + i conj(G1[k])
                    const float ykr = g0.x - g1.y, yki = g0.y + g1.x;
                    const float ymr = g0.x + g1.y, ymi = g1.x - g0.y;
                    // swap trick on input: feed (im, re)
                    s.xr[2 * u] = yki; s.xi[2 * u] = ykr;
                    s.xr[2 * u + 1] = ymi; s.xi[2 * u + 1] = ymr;
                }
            }
        });
    });

    wg_fft<P, f1_pack<P>(), 16>(ex, st, pl, lds,
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            const int g = tid / T, t = tid % T;
            float* l = lds + g * LF;
            const float* x = comp_of<comp>(s);
#pragma unroll
            for (int u = 0; u < EMAX / 2 + 1; ++u) {
                const int k = t + u * T;
                if (k < p.Cb) {
                    l[lpad(k)] = x[2 * u];
                    if (k != 0 && 2 * k != C) l[lpad(C - k)] = x[2 * u + 1];
                }
            }
        },
        [&](int tid, FftState& s, auto comp_c) {
            constexpr int comp = decltype(comp_c)::value;
            const int g = tid / T, t = tid % T;
            const float* l = lds + g * LF;
            float* o = comp_of<comp>(s);
            if (vec) {
#pragma unroll
                for (int q = 0; q < EMAX / 8; ++q) {
                    const int n0 = 8 * (t + q * T);
                    if (n0 < C) {
#pragma unroll
                        for (int c = 0; c < 8; ++c) o[q * 8 + c] = l[lpad(n0 + c)];
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < EMAX; ++q) {
                    const int n = t + q * T;
                    if (n < C) o[q] = l[lpad(n)];
                }
            }
        });

    ex.each(st, [&](int tid, FftState& s) {
        const int g = tid / T, t = tid % T;
        const int r0 = 2 * (bid * p.nb + g);
        uint32_t nan1 = 0, inf1 = 0, nan2 = 0, inf2 = 0;
        double ss = 0.0;
        // after the swap trick the true (re, im) = (xi, xr): row r0 = re, row r0+1 = im
        static_for<0, 2>([&](auto h_c) {
            constexpr int h = decltype(h_c)::value;
            const int row = r0 + h;
            if (row >= p.R) return;
            const float* x = comp_of<1 - h>(s);
            if (vec) {
                // the add-back loads of the row (16-bit base: the merge itself) go out together
                constexpr int NQ = EMAX / 8;
                const bool base16 = p.base && p.base_dtype != DT_F32;
                u32x4 braw[NQ];
                if (base16) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const int n0 = 8 * (t + q * T);
                        braw[q] = ((const u32x4*)p.base)[n0 < C ? ((size_t)row * C + n0) / 8 : 0];
                    }
                }
#pragma unroll
                for (int q = 0; q < EMAX / 8; ++q) {
                    const int n0 = 8 * (t + q * T);
                    if (n0 < C) {
                        const size_t off = (size_t)row * C + n0;
                        float o[8];
                        float bv[8];
                        if (base16) decode16x8(braw[q], p.base_dtype, bv);
                        else if (p.base) load_elem8(p.base, p.base_dtype, off, bv);
                        // fast path: no NaN/Inf anywhere in the group (an all-ones exponent is
                        // looked for with an and + max per value); otherwise the exact policy
                        uint32_t e1 = 0, e2 = 0;
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            const float v1 = x[q * 8 + c] * p.inv_n;
                            e1 = umax(e1, f2u(v1) & 0x7f800000u);
                            float v2 = v1 * p.post;
                            if (p.base) v2 += bv[c];
                            e2 = umax(e2, f2u(v2) & 0x7f800000u);
                            o[c] = v2;
                        }
                        if ((p.ifft_policy && e1 == 0x7f800000u) || e2 == 0x7f800000u) {
#pragma unroll
                            for (int c = 0; c < 8; ++c) {
                                float v = x[q * 8 + c] * p.inv_n;
                                if (p.ifft_policy) {
                                    if (is_nan(v)) { v = 0.f; nan1++; }
                                    if (is_inf(v)) inf1 = 1;
                                }
                                v *= p.post;
                                if (p.base) {
                                    v += bv[c];
                                    if (is_nan(v)) { v = 0.f; nan2++; }
                                    if (is_inf(v)) inf2 = 1;
                                }
                                o[c] = v;
                            }
                        }
                        if (p.norm_partials) {
                            float ps = 0.f;
#pragma unroll
                            for (int c = 0; c < 8; ++c) ps += o[c] * o[c];
                            ss += ps;
                        }
                        if (p.out_mode == OUT_BF16) {
                            u32x4 w;
                            w.x = pack_bf16x2(o[0], o[1]);
                            w.y = pack_bf16x2(o[2], o[3]);
                            w.z = pack_bf16x2(o[4], o[5]);
                            w.w = pack_bf16x2(o[6], o[7]);
                            ((u32x4*)p.out)[off / 8] = w;
                        } else {
                            cf4 w0 = {o[0], o[1], o[2], o[3]}, w1 = {o[4], o[5], o[6], o[7]};
                            ((cf4*)p.out)[off / 4] = w0;
                            ((cf4*)p.out)[off / 4 + 1] = w1;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < EMAX; ++q) {
                    const int n = t + q * T;
                    if (n < C) {
                        const size_t off = (size_t)row * C + n;
                        float v;
                        i2_finish(p, x[q], off, nan1, inf1, nan2, inf2, v);
                        ss += (double)v * v;
                        if (p.out_mode == OUT_BF16) ((uint16_t*)p.out)[off] = f_to_bf16(v);
                        else ((float*)p.out)[off] = v;
                    }
                }
            }
        });
        if (nan1) ex.global_atomic_add_u32(&p.flags[0], nan1);
        if (inf1) ex.global_atomic_or_u32(&p.flags[1], 1u);
        if (nan2) ex.global_atomic_add_u32(&p.flags[2], nan2);
        if (inf2) ex.global_atomic_or_u32(&p.flags[3], 1u);
        s.red[0] = ss; s.red[1] = 0.0;
    });
    if (p.norm_partials) {
        ex.sync();
        ex.template block_sum<2>(st, [&](const double* tot) {
            p.norm_partials[2 * (size_t)bid] = tot[0];
            p.norm_partials[2 * (size_t)bid + 1] = 0.0;
        });
    }
}

// =====================================================================
// A whole SLERP pair merge of two 1-D tensors in ONE work-group (R = 1, C <= PAIR1D_MAX_C): row
// transform (two-for-one), Hermitian split, both order statistics (three-level radix select in
// LDS), slerp sums and constants, blend, cull, inverse transform, scale / add-back / cast.  The
// multi-kernel pipeline spends ~25 launches (0.25 ms of launch latency) on such a tensor - every
// norm weight of a model.  Same arithmetic, same exact thresholds; sums in another order.
// =====================================================================
constexpr int PAIR1D_MAX_C = 8192;
struct Pair1dParams {
    FftPlanDev plan;            // N = C
    SigDesc a, b;               // role a = the larger-norm input
    int C;
    float sa, sb;               // 1 / ||a||, 1 / ||b||
    float t, t_sum;
    unsigned long long rank_cut; int have_cut;
    unsigned long long rank_cull; int have_cull;
    I2Params fin;               // inv_n, post, ifft_policy, base, out, flags, norm_partials (plan / G unused)
    float* thr;                 // [2]: cutoff and cull thresholds (device, as the selection passes leave them)
    BlendConsts* consts;
};

// k-th smallest (0-based, with multiplicities w) of the keys a thread holds: keys[j] for j < nk, two key
// sets (x: always, y: optional).  11 + 10 + 10 bits, histograms in LDS; every thread returns the key.
template <class Ex, class StT, class KeyFn>
SM_HD uint32_t wg_select_lds(Ex& ex, StT& st, uint32_t* hist, uint32_t* part, uint32_t* ctl, unsigned long long rank,
                             int per_thread, KeyFn keys) {
    using S = typename StT::value_type;
    const int nt = ex.nthreads();
    uint32_t prefix = 0;
    int prefix_bits = 0;
    unsigned long long r = rank;
    for (int level = 0; level < 3; ++level) {
        const int bits = level == 0 ? 11 : 10;
        const int nbins = 1 << bits;
        const int shift = 31 - prefix_bits - bits;
        ex.each(st, [&](int tid, S&) { for (int b = tid; b < nbins; b += nt) hist[b] = 0; });
        ex.sync();
        ex.each(st, [&](int tid, S& s) {
            for (int j = 0; j < per_thread; ++j) {
                uint32_t key[2], w;
                const int n = keys(tid, s, j, key, w);
                for (int e = 0; e < n; ++e)
                    if (prefix_bits == 0 || (key[e] >> (31 - prefix_bits)) == prefix)
                        ex.lds_atomic_add(&hist[(key[e] >> shift) & (uint32_t)(nbins - 1)], w);
            }
        });
        ex.sync();
        const int per = (nbins + nt - 1) / nt;
        const int ngrp = (nt + 15) / 16;
        uint32_t* grp = part + nt;                     // group totals of 16 threads' partials (counts fit 32 bits)
        ex.each(st, [&](int tid, S&) {
            uint32_t sum = 0;
            for (int q = 0; q < per; ++q) { const int b = tid * per + q; if (b < nbins) sum += hist[b]; }
            part[tid] = sum;
        });
        ex.sync();
        ex.each(st, [&](int tid, S&) {
            if (tid >= ngrp) return;
            uint32_t g = 0;
            for (int q = 0; q < 16; ++q) { const int i = tid * 16 + q; if (i < nt) g += part[i]; }
            grp[tid] = g;
        });
        ex.sync();
        // every thread finds where its own bins start (a few independent LDS reads); the one whose range
        // holds the rank walks its bins
        ex.each(st, [&](int tid, S&) {
            uint32_t excl = 0, total = 0;
            const int g0 = tid / 16;
            for (int g = 0; g < ngrp; ++g) { const uint32_t v = grp[g]; total += v; if (g < g0) excl += v; }
            for (int q = g0 * 16; q < tid; ++q) excl += part[q];
            if (total == 0) { if (tid == 0) { ctl[0] = 0; ctl[1] = 0; ctl[2] = 0; } return; }
            const uint32_t rr = r >= (unsigned long long)total ? total - 1u : (uint32_t)r;
            const uint32_t mine = part[tid];
            if (rr >= excl && rr - excl < mine) {
                uint32_t cum = excl;
                int b = tid * per;
                while (b < nbins - 1 && cum + hist[b] <= rr) { cum += hist[b]; ++b; }
                ctl[0] = (uint32_t)b; ctl[1] = rr - cum; ctl[2] = 0u;
            }
        });
        ex.sync();
        prefix = (prefix << bits) | ctl[0];
        prefix_bits += bits;
        r = (unsigned long long)ctl[1] | ((unsigned long long)ctl[2] << 32);
        ex.sync();
    }
    return prefix;
}

template <class P> constexpr bool pair1d_plan() {      // 1-D tensors go through this kernel up to PAIR1D_MAX_C elements only
    if constexpr (P::is_static) return P::N <= PAIR1D_MAX_C; else return true;
}
template <class P, class Ex>
SM_HD void k_pair1d(Ex& ex, const Pair1dParams& p) {
    if constexpr (!pair1d_plan<P>()) { return; } else {      // (the 16384- / 28672-point bodies were dead code with 594 spilled registers)
    typename Ex::template State<FftState> st;
    ex.init(st);
    const FftPlanDev& pl = p.plan;
    const int T = plan_T<P>(pl), C = plan_N<P>(pl);
    const int LF = plan_lds<P>(pl);
    const int Cb = C / 2 + 1;
    float* fftbuf = ex.lds() + LDS_SCRATCH_FLOATS;
    float* zr = fftbuf + LF;
    float* zi = zr + C;
    uint32_t* hist = (uint32_t*)(zi + C);
    uint32_t* part = hist + HIST1_BINS;             // nt words + nt / 16 group totals
    uint32_t* ctl = part + 1024 + 64;               // 8 words + the constants broadcast
    float* cbuf = (float*)(ctl + 8);
    const int QB = (Cb + T - 1) / T;                // bins per thread (<= EMAX / 2 + 1)

    // ---- forward: z = a + i b, one C-point transform, split by Hermitian symmetry ----
    // (straight-line on purpose: wrapping the two transforms / the two selections into loops to share
    //  their code made the 8192-point kernel spill 378 registers and 50 % slower)
    ex.each(st, [&](int tid, FftState& s) {
#pragma unroll
        for (int q = 0; q < EMAX; ++q) {
            const int n = tid + q * T;
            s.xr[q] = n < C ? load_sig1(p.a, (size_t)n) : 0.f;
            s.xi[q] = n < C ? load_sig1(p.b, (size_t)n) : 0.f;
        }
    });
    auto nat_scatter = [&](int tid, FftState& s, auto comp_c) {
        constexpr int comp = decltype(comp_c)::value;
        const float* x = comp_of<comp>(s);
#pragma unroll
        for (int q = 0; q < EMAX; ++q) { const int n = tid + q * T; if (n < C) fftbuf[lpad(n)] = x[q]; }
    };
    auto fin_gather = [&](int tid, FftState& s, auto comp_c) {
        constexpr int comp = decltype(comp_c)::value;
        float* o = comp_of<comp>(s);
#pragma unroll
        for (int q = 0; q < EMAX; ++q) { const int k = tid + q * T; if (k < C) o[q] = fftbuf[lpad(k)]; }
    };
    wg_fft<P>(ex, st, pl, fftbuf, nat_scatter, fin_gather);
    ex.each(st, [&](int tid, FftState& s) {
#pragma unroll
        for (int q = 0; q < EMAX; ++q) { const int k = tid + q * T; if (k < C) { zr[k] = s.xr[q]; zi[k] = s.xi[q]; } }
    });
    ex.sync();
    // bins k = tid + q T (q < QB): Re a -> xr[q], Im a -> xi[q], Re b -> xr[EMAX/2 + 1 + q]   (QB <= EMAX/2 + 1)
    constexpr int RB0 = EMAX / 2 + 1;
    ex.each(st, [&](int tid, FftState& s) {
        for (int q = 0; q < QB; ++q) {
            const int k = tid + q * T;
            float ra = 0.f, ia = 0.f, rb = 0.f;
            if (k < Cb) {
                const int m = (C - k) % C;
                const float r1 = zr[k], i1 = zi[k], r2 = zr[m], i2 = zi[m];
                ra = 0.5f * (r1 + r2) * p.sa; ia = 0.5f * (i1 - i2) * p.sa;
                rb = 0.5f * (i1 + i2) * p.sb;
            }
            s.xr[q] = ra; s.xi[q] = ia; s.xr[RB0 + q] = rb;
        }
    });
    ex.sync();

    // ---- cutoff threshold over |Re a| and |Re b| (functions.py:115-119) ----
    float thr0 = 0.f;
    if (p.have_cut) {
        const uint32_t key = wg_select_lds(ex, st, hist, part, ctl, p.rank_cut, QB,
            [&](int tid, FftState& s, int q, uint32_t* key2, uint32_t& w) {
                const int k = tid + q * T;
                if (k >= Cb) return 0;
                w = (uint32_t)bin_weight(k, C);
                key2[0] = f2u(s.xr[q]) & 0x7fffffffu; key2[1] = f2u(s.xr[RB0 + q]) & 0x7fffffffu;
                return 2;
            });
        thr0 = u2f(key);
    }
    // ---- slerp-class sums and constants (functions.py:36-43) ----
    ex.each(st, [&](int tid, FftState& s) {
        double s00 = 0, s01 = 0, s11 = 0, cnt = 0;
        for (int q = 0; q < QB; ++q) {
            const int k = tid + q * T;
            if (k >= Cb) continue;
            const float a = s.xr[q], b = s.xr[RB0 + q];
            if (same_sign(a, b) && !(fabsf(b) < thr0)) {
                const double w = (double)bin_weight(k, C);
                s00 += w * (double)(a * a); s01 += w * (double)(a * b); s11 += w * (double)(b * b); cnt += w;
            }
        }
        s.red[0] = s00; s.red[1] = s01; s.red[2] = s11; s.red[3] = cnt;
    });
    ex.template block_sum<4>(st, [&](const double* tot) {
        const double s00 = tot[0], s01 = tot[1], s11 = tot[2], cnt = tot[3];
        BlendConsts c;
        c.thr = thr0;
        c.s00 = s00; c.s01 = s01; c.s11 = s11; c.n_slerp = (unsigned long long)cnt;
        double dot = s01 / (sqrt(s00) * sqrt(s11));
        if (dot > 1.0) dot = 1.0;
        if (dot < -1.0) dot = -1.0;
        const float dotf = (float)dot;
        const float theta = acosf(dotf) * p.t;
        double rel2 = s11 - 2.0 * (double)dotf * s01 + (double)dotf * (double)dotf * s00;
        if (rel2 < 0) rel2 = 0;
        double reln = sqrt(rel2);
        if (reln < 1e-12) reln = 1e-12;
        c.dot = dotf; c.cos_t = cosf(theta); c.sin_t = sinf(theta); c.inv_rel = (float)(1.0 / reln);
        c.pad[0] = c.pad[1] = c.pad[2] = 0.f;
        *p.consts = c;
        p.thr[0] = thr0;
        cbuf[0] = c.dot; cbuf[1] = c.cos_t; cbuf[2] = c.sin_t; cbuf[3] = c.inv_rel;
    });
    BlendConsts bc;
    memset(&bc, 0, sizeof bc);
    bc.thr = thr0; bc.dot = cbuf[0]; bc.cos_t = cbuf[1]; bc.sin_t = cbuf[2]; bc.inv_rel = cbuf[3];
    // ---- blend (functions.py:121-145), cull threshold over |Re R| (:146-147) ----
    ex.each(st, [&](int tid, FftState& s) {
        for (int q = 0; q < QB; ++q) {
            const int k = tid + q * T;
            if (k < Cb) s.xr[q] = blend_slerp_one(bc, p.t_sum, s.xr[q], s.xr[RB0 + q]);
        }
    });
    ex.sync();
    float thr1 = 0.f;
    if (p.have_cull) {
        const uint32_t key = wg_select_lds(ex, st, hist, part, ctl, p.rank_cull, QB,
            [&](int tid, FftState& s, int q, uint32_t* key2, uint32_t& w) {
                const int k = tid + q * T;
                if (k >= Cb) return 0;
                w = (uint32_t)bin_weight(k, C);
                key2[0] = f2u(s.xr[q]) & 0x7fffffffu;
                return 1;
            });
        thr1 = u2f(key);
    }
    // ---- inverse: Hermitian extension of (Re R culled, Im a), swap trick, one C-point transform ----
    ex.each(st, [&](int tid, FftState& s) {
        if (tid == 0) p.thr[1] = thr1;
        for (int q = 0; q < QB; ++q) {
            const int k = tid + q * T;
            if (k < Cb) { float r = s.xr[q]; if (fabsf(r) < thr1) r = 0.f; zr[k] = r; zi[k] = s.xi[q]; }
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, FftState& s) {
#pragma unroll
        for (int q = 0; q < EMAX; ++q) {
            const int n = tid + q * T;
            float re = 0.f, im = 0.f;
            if (n < C) {
                if (n < Cb) { re = zr[n]; im = zi[n]; }
                else { re = zr[C - n]; im = -zi[C - n]; }
            }
            s.xr[q] = im; s.xi[q] = re;             // ifft(x) = swap(fft(swap(x)))
        }
    });
    ex.sync();
    wg_fft<P>(ex, st, pl, fftbuf, nat_scatter, fin_gather);
    ex.each(st, [&](int tid, FftState& s) {
        uint32_t nan1 = 0, inf1 = 0, nan2 = 0, inf2 = 0;
        double ss = 0.0;
#pragma unroll
        for (int q = 0; q < EMAX; ++q) {
            const int n = tid + q * T;
            if (n < C) {
                float v;
                i2_finish(p.fin, s.xi[q], (size_t)n, nan1, inf1, nan2, inf2, v);
                ss += (double)v * v;
                if (p.fin.out_mode == OUT_BF16) ((uint16_t*)p.fin.out)[n] = f_to_bf16(v);
                else ((float*)p.fin.out)[n] = v;
            }
        }
        if (nan1) ex.global_atomic_add_u32(&p.fin.flags[0], nan1);
        if (inf1) ex.global_atomic_or_u32(&p.fin.flags[1], 1u);
        if (nan2) ex.global_atomic_add_u32(&p.fin.flags[2], nan2);
        if (inf2) ex.global_atomic_or_u32(&p.fin.flags[3], 1u);
        s.red[0] = ss; s.red[1] = 0.0;
    });
    if (p.fin.norm_partials) {
        ex.sync();
        ex.template block_sum<2>(st, [&](const double* tot) { p.fin.norm_partials[0] = tot[0]; p.fin.norm_partials[1] = 0.0; });
    }
    }
}

// ---- kernel tags (sm_tag.hpp) ----
SM_FFT_KERNEL_TAG(KF1, F1Params, "f1_rows_fwd", k_f1<P>(ex, p), 1, 3)
SM_FFT_KERNEL_TAG(KF2, F2Params, "f2_cols_fwd", (k_f2<P, f2_bins<P>()>(ex, p)), 2 * f2_bins<P>(), 4)
SM_FFT_KERNEL_TAG(KI1x1, I1Params, "i1_cols_inv", (k_i1<P, 1>(ex, p)), 1, 4)
SM_FFT_KERNEL_TAG(KI1x2, I1Params, "i1_cols_inv", (k_i1<P, i1_bins<P>()>(ex, p)), i1_bins<P>(), 4)
SM_FFT_KERNEL_TAG(KI2, I2Params, "i2_rows_inv", k_i2<P>(ex, p), 1, 4)
SM_FFT_KERNEL_TAG(KF2S, F2SParams, "f2s_cols_fwd1", (k_f2s<P, f2s_groups<P>()>(ex, p)), f2s_groups<P>(), 4)
// radix-4 column step folded into the row pass (k_f1q) and its column-side companions
SM_FFT_KERNEL_TAG(KF1Q, F1Params, "f1_rows_fwd", k_f1q<P>(ex, p), 4, 4)
SM_FFT_KERNEL_TAG(KF2Q, F2Params, "f2_cols_fwd", (k_f2<P, f2_bins<P>(), true>(ex, p)), 2 * f2_bins<P>(), 4)
SM_FFT_KERNEL_TAG(KF2SQ, F2SParams, "f2s_cols_fwd1", (k_f2s<P, f2s_groups<P>(), true>(ex, p)), f2s_groups<P>(), 4)
SM_FFT_KERNEL_TAG(KI1x1Q, I1Params, "i1_cols_inv", (k_i1<P, 1, true>(ex, p)), 1, 4)
SM_FFT_KERNEL_TAG(KI1x2Q, I1Params, "i1_cols_inv", (k_i1<P, i1_bins<P>(), true>(ex, p)), i1_bins<P>(), 4)
SM_FFT_KERNEL_TAG(KPair1d, Pair1dParams, "pair_1d", k_pair1d<P>(ex, p), 1, 1)      // one work-group per launch: all the registers it wants
SM_KERNEL_TAG(KF2R1, F2Params, "f2_cols_fwd", k_f2_r1(ex, p))
SM_KERNEL_TAG(KI1R1, I1Params, "i1_cols_inv", k_i1_r1(ex, p))
// groups of smhip_side.hip (smhip_device.hpp): the _r1 column passes are this header's share of group 1; the
// run-time planned (DynPlan) transforms, the row passes and the 1-D pair merge one kernel per group
#define SM_KERNELS_R1(X) X(KF2R1) X(KI1R1)
#define SM_SIDE_KERNELS_3(X) X(KF1<DynPlan>)
#define SM_SIDE_KERNELS_17(X) X(KF1Q<DynPlan>)
#define SM_SIDE_KERNELS_18(X) X(KI2<DynPlan>)
#define SM_SIDE_KERNELS_19(X) X(KPair1d<DynPlan>)
#define SM_SIDE_KERNELS_4(X) X(KF2<DynPlan>) X(KF2Q<DynPlan>) X(KF2S<DynPlan>) X(KF2SQ<DynPlan>)
#define SM_SIDE_KERNELS_5(X) X(KI1x1<DynPlan>) X(KI1x2<DynPlan>) X(KI1x1Q<DynPlan>) X(KI1x2Q<DynPlan>)

}  // namespace smhip
