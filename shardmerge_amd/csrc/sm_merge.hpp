// sm_merge.hpp - the kernels of the spectral-merge pipeline around the transforms and the selection: the class blend,
// the spectral intermediates of rounds >= 2, the delta and serial norms, combine, AdditionMerge / TaskAdditionMerge,
// slerp and normalise at function level, correlate_pairs, the plane layout kernels, the DFT across the slices of a
// split column length and the transpose.  Where they stand in a pair merge: sm_kernels.hpp.
#pragma once
#include "sm_common.hpp"
#include "sm_tag.hpp"
#include "sm_select.hpp"         // (BlendConsts, CandLists)

namespace smhip {

enum { BLEND_SLERP = 0, BLEND_ARITH = 1 };
struct BlendParams {
    const float* reA; const float* reB;
    float* reR;
    int R, C, Cb;
    int vec4;
    int mode;
    int agreement;              // arithmetic branch: sign agreement on/off
    float t;                    // arithmetic: R = ra + t*rb
    float t_sum;
    const BlendConsts* consts;  // slerp mode
    unsigned long long* hist;   // level-1 histogram of |Re R| for the cull, or null
    int chunks;
};

SM_HD float blend_one(const BlendParams& p, const BlendConsts& c, float a, float b) {
    if (p.mode == BLEND_SLERP) {
        if (same_sign(a, b)) {
            if (fabsf(b) < c.thr) return a + p.t_sum * b;
            return a * c.cos_t + ((b - a * c.dot) * c.inv_rel) * c.sin_t;
        }
        return (fabsf(a) > fabsf(b)) ? a : b;
    }
    const bool agree = p.agreement ? same_sign(a, b) : true;
    return agree ? (a + p.t * b) : b;                 // quirk Q3: disagreeing bins take b
}

template <class Ex>
SM_HD void k_blend(Ex& ex, const BlendParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int nt = ex.nthreads();
    const size_t total = (size_t)p.Cb * p.R;
    const size_t nquad = (total + 3) / 4;
    BlendConsts c;
    memset(&c, 0, sizeof(c));
    if (p.mode == BLEND_SLERP) c = *p.consts;
    const WeightRanges wr = weight_ranges(p.R, p.C, p.Cb);
    if (p.hist) {
        ex.each(st, [&](int tid, EmptyState&) { for (int b = tid; b < HIST1_BINS; b += nt) lh[b] = 0; });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        auto quad = [&](size_t i0, const float* a, const float* b, int n, bool vec) {
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = blend_one(p, c, a[e], b[e]);
            if (vec) {
                cf4 v = {r[0], r[1], r[2], r[3]};
                *(cf4*)(p.reR + i0) = v;
            } else {
                for (int e = 0; e < n; ++e) p.reR[i0 + e] = r[e];
            }
            if (p.hist) {
                const uint32_t w0 = weight_at(wr, i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e < n) {
                        const uint32_t key = f2u(r[e]) & 0x7fffffffu;
                        ex.lds_atomic_add(&lh[key >> 20], (vec && !wr.full) ? w0 : weight_at(wr, i0 + e));
                    }
                }
            }
        };
        if (p.vec4) {
            // 16-byte loads of U steps in flight together (clamped, not branched around)
            constexpr int U = 4;
            const cf4* A4 = (const cf4*)p.reA;
            const cf4* B4 = (const cf4*)p.reB;
            for (int q0 = 0; q0 < p.chunks; q0 += U) {
                cf4 av[U], bv[U];
                size_t qv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    qv[u] = start + (size_t)(q0 + u) * nt + tid;
                    av[u] = A4[qv[u] < nquad ? qv[u] : nquad - 1];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) bv[u] = B4[qv[u] < nquad ? qv[u] : nquad - 1];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (q0 + u < p.chunks && qv[u] < nquad) {
                        const float a[4] = {av[u].x, av[u].y, av[u].z, av[u].w};
                        const float b[4] = {bv[u].x, bv[u].y, bv[u].z, bv[u].w};
                        quad(4 * qv[u], a, b, 4, true);
                    }
                }
            }
        } else {
            for (int q = 0; q < p.chunks; ++q) {
                const size_t qi = start + (size_t)q * nt + tid;
                if (qi >= nquad) break;
                float a[4], b[4];
                const int n = load_quad(p.reA, 4 * qi, total, 0, a);
                load_quad(p.reB, 4 * qi, total, 0, b);
                quad(4 * qi, a, b, n, false);
            }
        }
    });
    if (p.hist) {
        ex.sync();
        ex.each(st, [&](int tid, EmptyState&) {
            for (int b = tid; b < HIST1_BINS; b += nt) {
                const uint32_t v = lh[b];
                if (v) ex.global_atomic_add(&p.hist[b], (unsigned long long)v);
            }
        });
    }
}

// =====================================================================
// spectral intermediates (tournament rounds >= 2, DESIGN.md "K >= 3")
// =====================================================================
// A pair merge that is not the last leaves its result in the spectral domain: (Re R, Im a) with
// the cull still to be applied.  k_spec_norm takes || post * ifft(R) ||^2 * n / post^2 =
// sum over the FULL spectrum of |R_culled|^2 (Parseval), i.e. what the reference's torch.norm of
// the materialised intermediate measures (fast_fourier.py:209-210).
struct SpecNormParams {
    const float* re; const float* im;
    int R, C, Cb;
    int vec4;
    const float* thr;           // device scalar (cull threshold) or null
    double* partials;           // [grid][2]: sum w*re_c^2, sum w*im^2
    int chunks;
};
template <class Ex>
SM_HD void k_spec_norm(Ex& ex, const SpecNormParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t total = (size_t)p.Cb * p.R;
    const size_t nquad = (total + 3) / 4;
    const float thr = p.thr ? *p.thr : 0.f;
    const WeightRanges wr = weight_ranges(p.R, p.C, p.Cb);
    ex.each(st, [&](int tid, EmptyState& s) {
        double sr = 0, si = 0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int c = 0; c < p.chunks; ++c) {
            const size_t qi = start + (size_t)c * nt + tid;
            if (qi >= nquad) break;
            const size_t i0 = 4 * qi;
            float a[4], b[4];
            const int n = load_quad(p.re, i0, total, p.vec4, a);
            load_quad(p.im, i0, total, p.vec4, b);
            float qr = 0.f, qi2 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e < n) {
                    const float w = (float)weight_at(wr, i0 + e);
                    if (!(fabsf(a[e]) < thr)) qr += w * a[e] * a[e];
                    qi2 += w * b[e] * b[e];
                }
            }
            sr += qr; si += qi2;
        }
        s.red[0] = sr; s.red[1] = si;
    });
    ex.template block_sum<2>(st, [&](const double* tot) {
        p.partials[2 * (size_t)ex.bid()] = tot[0];
        p.partials[2 * (size_t)ex.bid() + 1] = tot[1];
    });
}

// the candidates' share of the Parseval sum once the cull threshold is known (sumsq above)
struct SumsqCandParams {
    CandLists cand;
    const float* thr;
    double* partials;          // [nblocks][4], appended after the selection pass's partials
};
template <class Ex>
SM_HD void k_sumsq_cand(Ex& ex, const SumsqCandParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const uint32_t n = p.cand.counters[2] ? 0u : p.cand.counters[0];
    const float thr = *p.thr;
    ex.each(st, [&](int tid, EmptyState& s) {
        double acc = 0;
        for (size_t q = (size_t)ex.bid() * nt + tid; q < n; q += (size_t)ex.nblocks() * nt) {
            const uint32_t v = p.cand.keys[q];
            const float x = u2f(v & 0x7fffffffu);
            if (!(x < thr)) acc += (double)(1u + (v >> 31)) * (double)x * (double)x;
        }
        s.red[0] = acc; s.red[1] = 0; s.red[2] = 0; s.red[3] = 0;
    });
    ex.template block_sum<4>(st, [&](const double* tot) {
        for (int q = 0; q < 4; ++q) p.partials[4 * (size_t)ex.bid() + q] = tot[q];
    });
}
// S_re = sum of partials[4i], S_im = sum of im_partials[i] -> out[0], out[1]; clears the list counters
struct SumSpecParams { const double* part4; int n4; const double* part1; int n1; double* out; uint32_t* zero_u32; int zero_u32_count; };
template <class Ex>
SM_HD void k_sum_spec(Ex& ex, const SumSpecParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState& s) {
        double a0 = 0, a1 = 0;
        for (int i = tid; i < p.n4; i += nt) a0 += p.part4[4 * (size_t)i];
        for (int i = tid; i < p.n1; i += nt) a1 += p.part1[i];
        if (p.zero_u32 && tid < p.zero_u32_count) p.zero_u32[tid] = 0u;
        s.red[0] = a0; s.red[1] = a1;
    });
    ex.template block_sum<2>(st, [&](const double* tot) { p.out[0] = tot[0]; p.out[1] = tot[1]; });
}

// Rounding-noise model.  In the reference an intermediate goes through ifft -> fft before the next
// round uses it, so the bins its cull zeroed come back as rounding noise (measured against the
// real reference, oracle/chaos_probe.py: Gaussian, sigma = 1.1e-7 .. 1.4e-7 of the rms bin of the
// unit-norm spectrum), and the next round takes its sign-agreement decisions and its 8 % quantile
// ON that noise.  Exact zeros there would change those decisions systematically (sign(0) = 0 never
// agrees; the quantile becomes 0), so the noise is modelled: a counter-based hash of
// (seed, element index) -> Box-Muller.  Only the statistics are reproducible by anyone - the
// reference does not reproduce its own noise across FFT libraries.
SM_HD uint32_t hash_u32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
SM_HD float model_noise(uint32_t seed, size_t i, float sigma) {
    const uint32_t h1 = hash_u32((uint32_t)i * 2u + 1u + seed * 0x9e3779b9u) ^ hash_u32((uint32_t)(i >> 31) + seed);
    const uint32_t h2 = hash_u32(h1 + 0x68bc21ebu);
    // 8 % of the reference's noise values are exact zeros (fp32 cancellation; sign(0) = 0 is its own
    // sign class there): measured 0.094 / 0.081 / 0.076 at 256^2 / 1024^2 / 4096^2
    if ((h2 >> 24) < 21u) return 0.f;
    // sum of four uniforms (variance 1/3): Gaussian enough - only the sign and the rank of a noise
    // value among the other noise values ever matter - and no transcendental in a streaming kernel
    const float s4 = (float)(h1 & 0xffffu) + (float)(h1 >> 16) + (float)(h2 & 0xffffu) + (float)(hash_u32(h2) >> 16);
    return sigma * 1.7320508f * (s4 * (1.0f / 65536.0f) - 2.0f);
}

struct SpecRescaleParams {
    const float* re; const float* im;   // the intermediate's planes (im may be null: role b)
    float* dre; float* dim;             // destination planes (may alias the sources)
    int R, C, Cb;
    int vec4;
    float thr;                          // cull threshold (value), applied on read
    float scale;                        // 1 / sqrt(sum |R_c|^2 / n): unit spatial norm
    float sigma; uint32_t seed;         // noise model for the culled bins
    unsigned long long* hist;           // level-1 histogram of |dre| or null
    int chunks;
    double* im_partials;                // role a (im != null) or null: [grid] sum w (Im written)^2
};
template <class Ex>
SM_HD void k_spec_rescale(Ex& ex, const SpecRescaleParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    uint32_t* lh = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);
    const int nt = ex.nthreads();
    const size_t total = (size_t)p.Cb * p.R;
    const size_t nquad = (total + 3) / 4;
    const WeightRanges wr = weight_ranges(p.R, p.C, p.Cb);
    if (p.hist) {
        ex.each(st, [&](int tid, EmptyState&) { for (int b = tid; b < HIST1_BINS; b += nt) lh[b] = 0; });
        ex.sync();
    }
    ex.each(st, [&](int tid, EmptyState& s) {
        double imacc = 0.0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int c = 0; c < p.chunks; ++c) {
            const size_t qi = start + (size_t)c * nt + tid;
            if (qi >= nquad) break;
            const size_t i0 = 4 * qi;
            float a[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            const int n = load_quad(p.re, i0, total, p.vec4, a);
            if (p.im) load_quad(p.im, i0, total, p.vec4, b);
            float r[4], im[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r[e] = (fabsf(a[e]) < p.thr) ? model_noise(p.seed, i0 + e, p.sigma) : a[e] * p.scale;
                im[e] = b[e] * p.scale;
            }
            if (p.vec4) {
                cf4 v = {r[0], r[1], r[2], r[3]};
                *(cf4*)(p.dre + i0) = v;
                if (p.im) { cf4 vi = {im[0], im[1], im[2], im[3]}; *(cf4*)(p.dim + i0) = vi; }
            } else {
                for (int e = 0; e < n; ++e) { p.dre[i0 + e] = r[e]; if (p.im) p.dim[i0 + e] = im[e]; }
            }
            if (p.hist) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) ex.lds_atomic_add(&lh[(f2u(r[e]) & 0x7fffffffu) >> 20], weight_at(wr, i0 + e));
            }
            if (p.im_partials) {
                float q = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) q += (float)weight_at(wr, i0 + e) * im[e] * im[e];
                imacc += q;
            }
        }
        s.red[0] = imacc;
    });
    if (p.hist) {
        ex.sync();
        ex.each(st, [&](int tid, EmptyState&) {
            for (int b = tid; b < HIST1_BINS; b += nt) {
                const uint32_t v = lh[b];
                if (v) ex.global_atomic_add(&p.hist[b], (unsigned long long)v);
            }
        });
    }
    if (p.im_partials) {
        ex.sync();
        ex.template block_sum<1>(st, [&](const double* tot) { p.im_partials[ex.bid()] = tot[0]; });
    }
}

// =====================================================================
// elementwise spatial kernels (deltas, norms, add branch, K=1 finish)
// =====================================================================
// ||finetune_i - base_i||^2 of every model in ONE pass (K >= 3 needs all norms before the
// first pairing): a base tensor shared by several models is loaded once per octet.
// 16-bit inputs, n % 8 == 0, 16-byte aligned pointers (the host falls back to k_combine otherwise).
constexpr int NORMS_MAX = 16;       // row length of the partials / mailbox
constexpr int NORMS_K = 8;          // models one launch handles
struct DeltaNormsParams {
    int k;                           // <= NORMS_K
    const void* ft[NORMS_K];
    const void* ubase[2];            // the (at most two) distinct base tensors
    int base_of[NORMS_K];            // model -> 0 / 1
    int dtype;
    size_t n;
    int chunks;                      // octets per thread
    double* partials;                // [grid][NORMS_MAX]
};
template <class Ex>
SM_HD void k_delta_norms(Ex& ex, const DeltaNormsParams& p) {
    typename Ex::template State<NormsState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t noct = p.n / 8;
    const u32x4* b0 = (const u32x4*)p.ubase[0];
    const u32x4* b1 = (const u32x4*)(p.ubase[1] ? p.ubase[1] : p.ubase[0]);
    ex.each(st, [&](int tid, NormsState& s) {
        double acc[NORMS_K];
#pragma unroll
        for (int i = 0; i < NORMS_K; ++i) acc[i] = 0.0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t oi = start + (size_t)q * nt + tid;
            if (oi >= noct) break;
            u32x4 rf[NORMS_K];
            const u32x4 r0 = b0[oi], r1 = b1[oi];
#pragma unroll
            for (int i = 0; i < NORMS_K; ++i) rf[i] = ((const u32x4*)p.ft[i < p.k ? i : 0])[oi];
            float v0[8], v1[8];
            decode16x8(r0, p.dtype, v0);
            decode16x8(r1, p.dtype, v1);
#pragma unroll
            for (int i = 0; i < NORMS_K; ++i) {
                float vf[8];
                decode16x8(rf[i], p.dtype, vf);
                const bool second = p.base_of[i] != 0;
                float ps = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = vf[e] - (second ? v1[e] : v0[e]);
                    ps += d * d;
                }
                if (i < p.k) acc[i] += ps;
            }
        }
#pragma unroll
        for (int i = 0; i < NORMS_MAX; ++i) s.red[i] = i < NORMS_K ? acc[i < NORMS_K ? i : 0] : 0.0;
    });
    ex.template block_sum<NORMS_MAX>(st, [&](const double* tot) {
        for (int i = 0; i < NORMS_MAX; ++i) p.partials[(size_t)ex.bid() * NORMS_MAX + i] = tot[i];
    });
}
// ---------------------------------------------------------------------------------
// norm_mode = reference_cpu: ||x||_2 exactly as torch.norm computes it on CPU for a contiguous
// fp32 tensor - acc = fma(x, x, acc) SERIALLY in 8 fp32 lanes (element i goes to lane i % 8),
// the lanes then added in order, sqrt.  That sum loses low bits once the running sum is large
// (-7e-4 at 16 M elements, -5e-3 at 67 M: oracle/norm_bias_probe.py), and the reference's
// pick-the-larger decisions (|ra| / ||a||  vs  |rb| / ||b||) follow the BIASED norms: an
// implementation with accurate norms differs from the reference's device=cpu output by 2e-2 on
// the merged delta at 8192^2 (profiles/parity_fullsize.json).  The chain is inherently sequential
// (n/8 dependent adds per lane: ~20 ms for 8192^2), so this mode is opt-in.
// One work-group per signal; wave 0's lanes 0..7 hold the accumulators, all waves stage squares
// of (x - base) through LDS, double-buffered.
// ---------------------------------------------------------------------------------
constexpr int SER_CHUNK = 4096;             // elements per staged chunk (512 rows of 8)
struct SerialNormParams {
    int k;
    SigDesc sig[16];
    size_t n;                               // n % 8 == 0
    float* out;                             // [k]: the fp32 norm torch would return
};
template <class Ex>
SM_HD void k_serial_norm(Ex& ex, const SerialNormParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    float* buf = ex.lds() + LDS_SCRATCH_FLOATS;          // two buffers of SER_CHUNK floats
    const int nt = ex.nthreads();
    const SigDesc sg = p.sig[ex.bid()];
    const size_t nchunks = (p.n + SER_CHUNK - 1) / SER_CHUNK;
    auto stage = [&](size_t c, int which) {
        ex.each(st, [&](int tid, EmptyState&) {
            float* dst = buf + which * SER_CHUNK;
            for (int o = tid; o < SER_CHUNK / 8; o += nt) {
                const size_t i0 = c * SER_CHUNK + (size_t)o * 8;
                float v[8];
                if (i0 < p.n) load_sig8(sg, i0, v);
                else { for (int e = 0; e < 8; ++e) v[e] = 0.f; }
#pragma unroll
                for (int e = 0; e < 8; ++e) dst[o * 8 + e] = v[e];               // acc = fma(x, x, acc): see sm_aten_norm.hpp
            }
        });
    };
    ex.each(st, [&](int, EmptyState& s) { s.red[0] = 0.0; });
    if (nchunks) stage(0, 0);
    ex.sync();
    for (size_t c = 0; c < nchunks; ++c) {
        const int cur = (int)(c & 1);
        if (c + 1 < nchunks) stage(c + 1, cur ^ 1);
        ex.each(st, [&](int tid, EmptyState& s) {
            if (tid < 8) {
                float acc = (float)s.red[0];
                const float* src = buf + cur * SER_CHUNK + tid;
                const size_t left = p.n - c * SER_CHUNK;
                const int rows = (int)((left < (size_t)SER_CHUNK ? left : (size_t)SER_CHUNK) / 8);
                int r = 0;
                for (; r + 16 <= rows; r += 16) {
                    float x[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) x[q] = src[(r + q) * 8];
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc = fmaf(x[q], x[q], acc);
                }
                for (; r < rows; ++r) acc = fmaf(src[r * 8], src[r * 8], acc);
                s.red[0] = (double)acc;
            }
        });
        ex.sync();
    }
    // lanes added in order, then the square root (fp32)
    float* lanes = buf;
    ex.each(st, [&](int tid, EmptyState& s) { if (tid < 8) lanes[tid] = (float)s.red[0]; });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0) {
            float tot = 0.f;
            for (int q = 0; q < 8; ++q) tot = tot + lanes[q];
            p.out[ex.bid()] = sqrtf(tot);
        }
    });
}

struct SumNParams { const double* partials; int nparts; double* out; };
template <class Ex>
SM_HD void k_sum_partials_n(Ex& ex, const SumNParams& p) {
    typename Ex::template State<NormsState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, NormsState& s) {
        double a[NORMS_MAX];
#pragma unroll
        for (int i = 0; i < NORMS_MAX; ++i) a[i] = 0.0;
        for (int r = tid; r < p.nparts; r += nt) {
#pragma unroll
            for (int i = 0; i < NORMS_MAX; ++i) a[i] += p.partials[(size_t)r * NORMS_MAX + i];
        }
#pragma unroll
        for (int i = 0; i < NORMS_MAX; ++i) s.red[i] = a[i];
    });
    ex.template block_sum<NORMS_MAX>(st, [&](const double* tot) {
        for (int i = 0; i < NORMS_MAX; ++i) p.out[i] = tot[i];
    });
}

struct CombineParams {
    SigDesc a, b;               // b.x may be null
    float ca, cb;               // out = ca*a + cb*b
    size_t n;
    int vec8;                   // n % 8 == 0 and every pointer 16-byte aligned
    float* out_f32;             // or null (norms only)
    // optional finish: add base, NaN/Inf policy, bf16 / f32 store
    const void* base; int base_dtype;
    void* out_final; int out_mode;
    uint32_t* flags;
    double* partials;           // [grid][2] sum a^2, sum b^2 (of the un-weighted signals) or null
    int chunks;                 // octets per thread
};

template <class Ex>
SM_HD void k_combine(Ex& ex, const CombineParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t noct = (p.n + 7) / 8;
    ex.each(st, [&](int tid, EmptyState& s) {
        double sa = 0, sb = 0;
        uint32_t nan2 = 0, inf2 = 0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        // 16-bit inputs, no finishing stage (the norms of the raw deltas, K >= 3): the loads of
        // U octets go out together, clamped instead of branched around, and are decoded afterwards
        const bool fast16 = p.vec8 && !p.out_final && p.a.x && p.a.dtype != DT_F32 && (!p.b.x || p.b.dtype != DT_F32);
        if (fast16) {
            constexpr int U = 4;
            const bool has_ab = p.a.base != nullptr, has_b = p.b.x != nullptr, has_bb = has_b && p.b.base != nullptr;
            const u32x4* pa = (const u32x4*)p.a.x;
            const u32x4* pab = has_ab ? (const u32x4*)p.a.base : pa;
            const u32x4* pb = has_b ? (const u32x4*)p.b.x : pa;
            const u32x4* pbb = has_bb ? (const u32x4*)p.b.base : pa;
            for (int q0 = 0; q0 < p.chunks; q0 += U) {
                u32x4 ra[U], rab[U], rb[U], rbb[U];
                size_t oc[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const size_t oi = start + (size_t)(q0 + u) * nt + tid;
                    ok[u] = (q0 + u) < p.chunks && oi < noct;
                    oc[u] = ok[u] ? oi : 0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) ra[u] = pa[oc[u]];
#pragma unroll
                for (int u = 0; u < U; ++u) rab[u] = pab[oc[u]];
#pragma unroll
                for (int u = 0; u < U; ++u) rb[u] = pb[oc[u]];
#pragma unroll
                for (int u = 0; u < U; ++u) rbb[u] = pbb[oc[u]];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (!ok[u]) continue;
                    float va[8], ba[8], vb[8], bb[8], o[8];
                    decode16x8(ra[u], p.a.dtype, va); decode16x8(rab[u], p.a.dtype, ba);
                    decode16x8(rb[u], p.b.dtype, vb); decode16x8(rbb[u], p.b.dtype, bb);
                    float pa2 = 0.f, pb2 = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float xa = (va[e] - (has_ab ? ba[e] : 0.f)) * p.a.prescale;
                        const float xb = has_b ? (vb[e] - (has_bb ? bb[e] : 0.f)) * p.b.prescale : 0.f;
                        pa2 += xa * xa; pb2 += xb * xb;
                        o[e] = p.ca * xa + (has_b ? p.cb * xb : 0.f);
                    }
                    sa += pa2; sb += pb2;
                    if (p.out_f32) {
                        cf4 w0 = {o[0], o[1], o[2], o[3]}, w1 = {o[4], o[5], o[6], o[7]};
                        ((cf4*)p.out_f32)[2 * oc[u]] = w0; ((cf4*)p.out_f32)[2 * oc[u] + 1] = w1;
                    }
                }
            }
        }
        for (int q = 0; q < (fast16 ? 0 : p.chunks); ++q) {
            const size_t oi = start + (size_t)q * nt + tid;
            if (oi >= noct) break;
            const size_t i0 = 8 * oi;
            float a[8], b[8], bs[8], o[8];
            int cnt = 8;
            if (p.vec8) {
                load_sig8(p.a, i0, a);
                load_sig8(p.b, i0, b);
                if (p.out_final && p.base) load_elem8(p.base, p.base_dtype, i0, bs);
            } else {
                cnt = (int)((p.n - i0) < 8 ? (p.n - i0) : 8);
                for (int e = 0; e < 8; ++e) {
                    a[e] = b[e] = bs[e] = 0.f;
                    if (e < cnt) {
                        a[e] = load_sig1(p.a, i0 + e); b[e] = load_sig1(p.b, i0 + e);
                        if (p.out_final && p.base) bs[e] = load_elem(p.base, p.base_dtype, i0 + e);
                    }
                }
            }
            float pa = 0.f, pb = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                pa += a[e] * a[e]; pb += b[e] * b[e];
                float v = p.ca * a[e] + (p.b.x ? p.cb * b[e] : 0.f);
                o[e] = v;
            }
            sa += pa; sb += pb;
            if (p.out_f32) {
                if (p.vec8) {
                    cf4 w0 = {o[0], o[1], o[2], o[3]}, w1 = {o[4], o[5], o[6], o[7]};
                    ((cf4*)p.out_f32)[i0 / 4] = w0; ((cf4*)p.out_f32)[i0 / 4 + 1] = w1;
                } else {
                    for (int e = 0; e < cnt; ++e) p.out_f32[i0 + e] = o[e];
                }
            }
            if (p.out_final) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = o[e];
                    if (p.base) v += bs[e];
                    if (e < cnt) {
                        if (is_nan(v)) { v = 0.f; nan2++; }
                        if (is_inf(v)) inf2 = 1;
                    }
                    o[e] = v;
                }
                if (p.vec8 && p.out_mode == OUT_BF16) {
                    u32x4 w;
                    w.x = (uint32_t)f_to_bf16(o[0]) | ((uint32_t)f_to_bf16(o[1]) << 16);
                    w.y = (uint32_t)f_to_bf16(o[2]) | ((uint32_t)f_to_bf16(o[3]) << 16);
                    w.z = (uint32_t)f_to_bf16(o[4]) | ((uint32_t)f_to_bf16(o[5]) << 16);
                    w.w = (uint32_t)f_to_bf16(o[6]) | ((uint32_t)f_to_bf16(o[7]) << 16);
                    ((u32x4*)p.out_final)[oi] = w;
                } else {
                    for (int e = 0; e < cnt; ++e) {
                        if (p.out_mode == OUT_BF16) ((uint16_t*)p.out_final)[i0 + e] = f_to_bf16(o[e]);
                        else ((float*)p.out_final)[i0 + e] = o[e];
                    }
                }
            }
        }
        s.red[0] = sa; s.red[1] = sb;
        if (nan2) ex.global_atomic_add_u32(&p.flags[2], nan2);
        if (inf2) ex.global_atomic_or_u32(&p.flags[3], 1u);
    });
    if (p.partials) {
        ex.template block_sum<2>(st, [&](const double* tot) {
            p.partials[2 * (size_t)ex.bid()] = tot[0];
            p.partials[2 * (size_t)ex.bid() + 1] = tot[1];
        });
    }
}

// =====================================================================
// A1 / A8 at function level (not on the merge's hot path - inside it both are fused into the kernels above):
// slerp(v0, v1, t) (reference shard/tensor/functions.py:24-43) and tensor / norm (functions.py:75-88).
//   dot   = clamp(sum(v0 v1) / (||v0|| ||v1||), -1, 1)        (quirk Q5: the cosine of the UN-normalised vectors)
//   theta = acos(dot) t;  rel = v1 - v0 dot;  rel /= max(||rel||_2 along the LAST dim, 1e-12)   (F.normalize(dim=-1))
//   out   = v0 cos(theta) + rel sin(theta)
// Sums are taken in fp64 and rounded once (torch sums in fp32: the two agree to a few 1e-8), the element-wise
// part is torch's sequence of fp32 operations.
// =====================================================================
struct FnSumsParams { const float* v0; const float* v1; size_t n; int chunks; double* partials; };   // [grid][4]
template <class Ex>
SM_HD void k_fn_sums(Ex& ex, const FnSumsParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState& s) {
        double s01 = 0, s00 = 0, s11 = 0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int c = 0; c < p.chunks; ++c) {
            const size_t i = start + (size_t)c * nt + tid;
            if (i >= p.n) break;
            const double a = (double)p.v0[i], b = (double)p.v1[i];
            s01 += a * b; s00 += a * a; s11 += b * b;
        }
        s.red[0] = s01; s.red[1] = s00; s.red[2] = s11; s.red[3] = 0.0;
    });
    ex.template block_sum<4>(st, [&](const double* tot) {
        for (int q = 0; q < 4; ++q) p.partials[4 * (size_t)ex.bid() + q] = tot[q];
    });
}
SM_HD float fn_acosf(float x) { return acosf(x); }
struct FnSlerpFinParams { const double* partials; int nparts; float t; float* consts; };    // consts: dot, cos(theta), sin(theta), -
template <class Ex>
SM_HD void k_fn_slerp_fin(Ex& ex, const FnSlerpFinParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState& s) {
        double a = 0, b = 0, c = 0;
        for (int i = tid; i < p.nparts; i += nt) { a += p.partials[4 * i]; b += p.partials[4 * i + 1]; c += p.partials[4 * i + 2]; }
        s.red[0] = a; s.red[1] = b; s.red[2] = c; s.red[3] = 0.0;
    });
    ex.template block_sum<4>(st, [&](const double* tot) {
        // (0 / 0 = NaN for a zero vector, as in the reference: clamp keeps NaN)
        float dot = (float)tot[0] / ((float)sqrt(tot[1]) * (float)sqrt(tot[2]));
        if (dot < -1.f) dot = -1.f;
        if (dot > 1.f) dot = 1.f;
        const float theta = fn_acosf(dot) * p.t;
        p.consts[0] = dot; p.consts[1] = cosf(theta); p.consts[2] = sinf(theta); p.consts[3] = 0.f;
    });
}
// one work-group per (row, column segment).  PHASE 0: sum of rel^2 of the segment -> part[row * cchunks + seg];
// PHASE 1: the outputs
struct FnSlerpRowsParams {
    const float* v0; const float* v1; float* out;
    size_t rows, cols;
    int cchunks, seg;               // segments per row, elements per segment
    const float* consts;
    double* part;                   // [rows * cchunks]
    const float* den;               // [rows]: max(||rel row||, 1e-12)
};
template <int PHASE, class Ex>
SM_HD void k_fn_slerp_rows(Ex& ex, const FnSlerpRowsParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t row = (size_t)ex.bid() / p.cchunks;
    const int sg = (int)((size_t)ex.bid() % p.cchunks);
    const float dot = p.consts[0], ct = p.consts[1], sn = p.consts[2];
    const size_t c0 = (size_t)sg * p.seg, c1 = (c0 + p.seg < p.cols) ? c0 + p.seg : p.cols;
    const float dn = PHASE == 1 ? p.den[row] : 1.f;
    ex.each(st, [&](int tid, EmptyState& s) {
        double acc = 0.0;
        for (size_t c = c0 + tid; c < c1; c += nt) {
            const size_t i = row * p.cols + c;
            const float a = p.v0[i];
            const float rel = aten_fadd_(p.v1[i], -aten_fmul_(a, dot));
            if (PHASE == 0) acc += (double)rel * (double)rel;
            else p.out[i] = aten_fadd_(aten_fmul_(a, ct), aten_fmul_(rel / dn, sn));
        }
        s.red[0] = acc;
    });
    if (PHASE == 0) ex.template block_sum<1>(st, [&](const double* tot) { p.part[row * p.cchunks + sg] = tot[0]; });
}
struct FnSlerpDenParams { const double* part; size_t rows; int cchunks; float* den; };
template <class Ex>
SM_HD void k_fn_slerp_den(Ex& ex, const FnSlerpDenParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t row = (size_t)ex.bid() * ex.nthreads() + tid;
        if (row >= p.rows) return;
        double a = 0.0;
        for (int c = 0; c < p.cchunks; ++c) a += p.part[row * p.cchunks + c];
        const float nrm = (float)sqrt(a);
        p.den[row] = nrm > 1e-12f ? nrm : 1e-12f;
    });
}
// sum of squares of a tensor of any dtype (the exact norm of normalize_tensor) -> partials [grid][2] (k_sum_partials' layout)
struct SumsqAnyParams { const void* x; int dtype; size_t n; int chunks; double* partials; };
template <class Ex>
SM_HD void k_sumsq_any(Ex& ex, const SumsqAnyParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState& s) {
        double a = 0.0;
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int c = 0; c < p.chunks; ++c) {
            const size_t i = start + (size_t)c * nt + tid;
            if (i >= p.n) break;
            const double v = (double)load_elem(p.x, p.dtype, i);
            a += v * v;
        }
        s.red[0] = a; s.red[1] = 0.0;
    });
    ex.template block_sum<2>(st, [&](const double* tot) { p.partials[2 * (size_t)ex.bid()] = tot[0]; p.partials[2 * (size_t)ex.bid() + 1] = tot[1]; });
}
// out = x / s in x's dtype: a 16-bit tensor divided by a Python float is an fp32 division rounded to the dtype
struct DivScalarParams { const void* x; void* out; int dtype; size_t n; float s; int chunks; };
template <class Ex>
SM_HD void k_div_scalar(Ex& ex, const DivScalarParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int c = 0; c < p.chunks; ++c) {
            const size_t i = start + (size_t)c * nt + tid;
            if (i >= p.n) break;
            const float v = load_elem(p.x, p.dtype, i) / p.s;
            if (p.dtype == DT_F32) ((float*)p.out)[i] = v;
            else if (p.dtype == DT_BF16) ((uint16_t*)p.out)[i] = f_to_bf16_any(v);
            else ((uint16_t*)p.out)[i] = f_to_f16_any(v);
        }
    });
}

// =====================================================================
// N3: AdditionMerge / TaskAdditionMerge (reference shard/merge/addition.py:70-76,
// taskaddition.py:69-79) - sums of finetune deltas relative to output_base_model's tensor,
// in the TENSORS' dtype as torch computes it on CPU: a 16-bit elementwise op is an fp32 op
// rounded to the dtype, a 16-bit sum over the stacked dim accumulates in fp32 and rounds once.
//   mode 0 (AdditionMerge):      out = 0; for each ft: out = rnd(out + rnd(ft - base))
//   mode 1 (TaskAdditionMerge):  d_i = rnd(ft_i - base); s = sign(sum_i sign(d_i));
//                                out = rnd(sum_i d_i * [sign(d_i) == s])
// Neither adds the base back (the reference does not).
// =====================================================================
constexpr int ADD_MAX_MODELS = 16;
struct AdditionParams {
    int k;
    const void* ft[ADD_MAX_MODELS];
    const void* base;
    int dtype;
    size_t n;
    int mode;                   // 0: AdditionMerge, 1: TaskAdditionMerge
    void* out;                  // dtype, [n]
    int vec8;                   // n % 8 == 0 and 16-byte aligned pointers
    int chunks;                 // octets per thread
};
template <class Ex>
SM_HD void k_addition(Ex& ex, const AdditionParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t noct = (p.n + 7) / 8;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t oi = start + (size_t)q * nt + tid;
            if (oi >= noct) break;
            const size_t i0 = 8 * oi;
            const int cnt = p.vec8 ? 8 : (int)((p.n - i0) < 8 ? (p.n - i0) : 8);
            float b[8], acc[8], ssum[8];
            auto load8 = [&](const void* src, float* dst) {
                if (p.vec8) { load_elem8(src, p.dtype, i0, dst); return; }
                for (int e = 0; e < 8; ++e) dst[e] = e < cnt ? load_elem(src, p.dtype, i0 + e) : 0.f;
            };
            load8(p.base, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) { acc[e] = 0.f; ssum[e] = 0.f; }
            if (p.mode == 0) {
                for (int i = 0; i < p.k; ++i) {
                    float f[8];
                    load8(p.ft[i], f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = round_to_dtype(acc[e] + round_to_dtype(f[e] - b[e], p.dtype), p.dtype);
                }
            } else {
                for (int i = 0; i < p.k; ++i) {                  // pass 1: the majority sign
                    float f[8];
                    load8(p.ft[i], f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) ssum[e] += sign_of(round_to_dtype(f[e] - b[e], p.dtype));
                }
                for (int i = 0; i < p.k; ++i) {                  // pass 2: masked sum (the inputs come from L2 now)
                    float f[8];
                    load8(p.ft[i], f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float d = round_to_dtype(f[e] - b[e], p.dtype);
                        const float keep = (sign_of(d) == sign_of(round_to_dtype(ssum[e], p.dtype))) ? 1.f : 0.f;
                        acc[e] += round_to_dtype(d * keep, p.dtype);   // NaN * 0 = NaN, as in the reference
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = round_to_dtype(acc[e], p.dtype);
            }
            if (p.dtype == DT_F32) {
                if (p.vec8) {
                    cf4 w0 = {acc[0], acc[1], acc[2], acc[3]}, w1 = {acc[4], acc[5], acc[6], acc[7]};
                    ((cf4*)p.out)[i0 / 4] = w0; ((cf4*)p.out)[i0 / 4 + 1] = w1;
                } else {
                    for (int e = 0; e < cnt; ++e) ((float*)p.out)[i0 + e] = acc[e];
                }
            } else {
                uint16_t h[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) h[e] = p.dtype == DT_BF16 ? f_to_bf16_any(acc[e]) : f_to_f16_any(acc[e]);
                if (p.vec8) {
                    u32x4 w;
                    w.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16); w.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
                    w.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16); w.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
                    ((u32x4*)p.out)[oi] = w;
                } else {
                    for (int e = 0; e < cnt; ++e) ((uint16_t*)p.out)[i0 + e] = h[e];
                }
            }
        }
    });
}

// =====================================================================
// correlate_pairs (reference shard/tensor/functions.py:304-314; used by the legacy fourier.py
// operator's pairing): matrix[i][j] = mean over the trailing positions of
// cosine_similarity(t_i, t_j, dim=0).nan_to_num(0).  The tensors are viewed as [rows = shape[0]]
// x [cols = the rest]; one thread owns a column and walks a slice of the rows (coalesced across
// the lanes); partial sums of the K(K+1)/2 products go to a workspace, a second kernel finishes.
// =====================================================================
constexpr int CORR_MAX_K = 8;
constexpr int CORR_MAX_P = CORR_MAX_K * (CORR_MAX_K + 1) / 2;
struct CorrPartialParams {
    int k;
    const void* t[CORR_MAX_K];
    int dtype;
    size_t rows, cols;
    int splits;                 // row slices (grid y)
    double* part;               // [splits][P][cols]
};
SM_HD int corr_pair_index(int i, int j, int k) { return i * k - i * (i - 1) / 2 + (j - i); }     // i <= j
template <class Ex>
SM_HD void k_corr_partial(Ex& ex, const CorrPartialParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t cblocks = (p.cols + nt - 1) / nt;
    const size_t cb = (size_t)ex.bid() % cblocks, sp = (size_t)ex.bid() / cblocks;
    const int P = p.k * (p.k + 1) / 2;
    const size_t r0 = p.rows * sp / p.splits, r1 = p.rows * (sp + 1) / p.splits;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t c = cb * nt + tid;
        if (c >= p.cols) return;
        double acc[CORR_MAX_P];
#pragma unroll
        for (int q = 0; q < CORR_MAX_P; ++q) acc[q] = 0.0;
        for (size_t r = r0; r < r1; ++r) {
            float v[CORR_MAX_K];
#pragma unroll
            for (int i = 0; i < CORR_MAX_K; ++i) v[i] = i < p.k ? load_elem(p.t[i], p.dtype, r * p.cols + c) : 0.f;
            int q = 0;
#pragma unroll
            for (int i = 0; i < CORR_MAX_K; ++i) {
#pragma unroll
                for (int j = i; j < CORR_MAX_K; ++j) {
                    if (i < p.k && j < p.k) acc[q] += (double)v[i] * (double)v[j];
                    if (j < p.k) ++q;            // q runs over the pairs of the first k tensors only
                }
            }
        }
        int q = 0;
        for (int i = 0; i < p.k; ++i)
            for (int j = i; j < p.k; ++j, ++q) p.part[((size_t)sp * P + q) * p.cols + c] = acc[q];
    });
}
struct CorrFinishParams {
    int k;
    size_t cols;
    int splits;
    const double* part;
    float eps;                  // torch.nn.functional.cosine_similarity: 1e-8
    float* out;                 // [k][k], host-mapped
};
template <class Ex>
SM_HD void k_corr_finish(Ex& ex, const CorrFinishParams& p) {
    // one work-group per pair (i < j)
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int P = p.k * (p.k + 1) / 2;
    int pi = 0, pj = 0, cnt = 0;
    for (int i = 0; i < p.k; ++i)
        for (int j = i + 1; j < p.k; ++j, ++cnt)
            if (cnt == ex.bid()) { pi = i; pj = j; }
    const int qij = corr_pair_index(pi, pj, p.k), qii = corr_pair_index(pi, pi, p.k), qjj = corr_pair_index(pj, pj, p.k);
    ex.each(st, [&](int tid, EmptyState& s) {
        double sum = 0.0;
        for (size_t c = tid; c < p.cols; c += nt) {
            double dij = 0, dii = 0, djj = 0;
            for (int sp = 0; sp < p.splits; ++sp) {
                dij += p.part[((size_t)sp * P + qij) * p.cols + c];
                dii += p.part[((size_t)sp * P + qii) * p.cols + c];
                djj += p.part[((size_t)sp * P + qjj) * p.cols + c];
            }
            const double ni = sqrt(dii), nj = sqrt(djj);
            float cosv = (float)(dij / ((ni > p.eps ? ni : (double)p.eps) * (nj > p.eps ? nj : (double)p.eps)));
            if (is_nan(cosv)) cosv = 0.f;                                    // nan_to_num(0)
            else if (is_inf(cosv)) cosv = cosv > 0 ? 3.4028234663852886e38f : -3.4028234663852886e38f;
            sum += cosv;
        }
        s.red[0] = sum;
    });
    ex.template block_sum<1>(st, [&](const double* tot) {
        const float m = (float)(tot[0] / (double)p.cols);
        p.out[pi * p.k + pj] = m;
        p.out[pj * p.k + pi] = m;
    });
}

// expand half-spectrum planes to the full complex spectrum (test / API helper:
// the reference's fft_transform returns all R x C bins)
struct ExpandParams {
    const float* re; const float* im;   // planes [Cb][R]
    int R, C, Cb;
    cf2* full;                          // [R][C]
    int chunks;
};
template <class Ex>
SM_HD void k_expand(Ex& ex, const ExpandParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t total = (size_t)p.R * p.C;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t i = start + (size_t)q * nt + tid;
            if (i >= total) break;
            const int r = (int)(i / p.C), k = (int)(i % p.C);
            cf2 v;
            if (k < p.Cb) {
                v.x = p.re[(size_t)k * p.R + r]; v.y = p.im[(size_t)k * p.R + r];
            } else {
                const int kk = p.C - k, rr = (p.R - r) % p.R;
                v.x = p.re[(size_t)kk * p.R + rr]; v.y = -p.im[(size_t)kk * p.R + rr];
            }
            p.full[i] = v;
        }
    });
}

// gather a full complex spectrum [R][C] (interleaved) into half-spectrum planes
// [Cb][R].  sym = 1 first projects onto the Hermitian part, which is what taking
// `.real` of the inverse transform does (reference functions.py:71-73).
struct PackParams {
    const cf2* full; int R, C, Cb;
    float* re; float* im;
    int sym;
    int chunks;
};
template <class Ex>
SM_HD void k_pack(Ex& ex, const PackParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const size_t total = (size_t)p.Cb * p.R;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t i = start + (size_t)q * nt + tid;
            if (i >= total) break;
            const int k = (int)(i / p.R), r = (int)(i % p.R);
            cf2 v = p.full[(size_t)r * p.C + k];
            if (p.sym) {
                const int rr = (p.R - r) % p.R, kk = (p.C - k) % p.C;
                const cf2 m = p.full[(size_t)rr * p.C + kk];
                v.x = 0.5f * (v.x + m.x); v.y = 0.5f * (v.y - m.y);
            }
            p.re[i] = v.x; p.im[i] = v.y;
        }
    });
}

// interleaved complex <-> two planes in the same (row-major) order; cull in place
struct SplitParams { const cf2* full; float* re; float* im; size_t n; int chunks; };
template <class Ex>
SM_HD void k_split(Ex& ex, const SplitParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t i = start + (size_t)q * nt + tid;
            if (i >= p.n) break;
            const cf2 v = p.full[i];
            p.re[i] = v.x; p.im[i] = v.y;
        }
    });
}
struct JoinParams { const float* re; const float* im; cf2* full; size_t n; int chunks; };
template <class Ex>
SM_HD void k_join(Ex& ex, const JoinParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t i = start + (size_t)q * nt + tid;
            if (i >= p.n) break;
            cf2 v = {p.re[i], p.im[i]};
            p.full[i] = v;
        }
    });
}
struct CullParams { float* x; size_t n; const float* thr; int chunks; };
template <class Ex>
SM_HD void k_cull(Ex& ex, const CullParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const float thr = *p.thr;
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t start = (size_t)ex.bid() * p.chunks * nt;
        for (int q = 0; q < p.chunks; ++q) {
            const size_t i = start + (size_t)q * nt + tid;
            if (i >= p.n) break;
            if (fabsf(p.x[i]) < thr) p.x[i] = 0.f;
        }
    });
}


// =====================================================================
// Long / rough column lengths: R = p * M with M a length the work-group engine plans
// (even) and p <= DFTP_MAX_P anything (43 for the 11008 of Llama-2-7B, 37 for the 18944 of
// Qwen2-7B, 2 for 65536 ...).  Decimation in frequency with n = n1 + M n2, k = p k1 + k2:
//
//     X[p k1 + k2] = sum_n1 W_M^(n1 k1) * { W_R^(n1 k2) * sum_n2 W_p^(n2 k2) x[n1 + M n2] }
//
// so the p row BLOCKS [n2 M, (n2+1) M) are first combined by a p-point DFT (this kernel, in
// place on the row pass's output T1, with the W_R twiddle), and block k2 then goes through
// the ordinary M-point column pass - the pipeline treats the tensor as p slices of M rows
// (the `batch` machinery) whose planes hold the bins k = p k1 + k2 of slice k2.  The inverse
// runs the other way round: M-point inverse column passes per slice, then the conjugate
// twiddle and the inverse p-point DFT across the slices of G, then the inverse row pass.
// The direct p-point sums cost O(p) per element: HBM-bound up to p ~ 16, ALU-bound beyond.
// =====================================================================
constexpr int DFTP_MAX_P = 256;
constexpr int DFTP_COLS = 16;          // bin columns per work-group: 16 x 16 B = 256 contiguous bytes
constexpr int DFTP_KB = 4;             // outputs a thread accumulates together
struct DftpParams {
    cf4* buf;              // T1 (forward) or G (inverse): p slices
    const cf2* tw;         // tw[j] = exp(-2 pi i j / (p M)), j < p M
    int p, M;
    int units;             // row units per slice: M (a cf4 = signals a, b of one row) or M / 2 (rowpair)
    int rowpair;           // 1: a cf4 = rows 2u, 2u + 1 of ONE signal (their twiddles differ)
    int ilv;               // rows interleaved in groups of ilv (T1 of the two-signal row pass)
    int pitch;             // cf4 per row unit
    int ncols;             // valid bin columns
    size_t slice_stride;   // cf4 between slices
    int inverse;
    int cols;              // k_dftp_pairs: bin columns per work-group (16 ... 128; the fewer outputs per column - small p -
                           // the more columns share a work-group)
};
SM_HD cf2 cmul(cf2 a, cf2 b) { cf2 r = {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; return r; }
template <class Ex>
SM_HD void k_dftp(Ex& ex, const DftpParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    cf4* tile = (cf4*)(ex.lds() + LDS_SCRATCH_FLOATS);             // [p][DFTP_COLS]
    cf2* wp = (cf2*)(tile + (size_t)p.p * DFTP_COLS);               // W_p^j (conjugated for the inverse)
    const int ntiles = (p.ncols + DFTP_COLS - 1) / DFTP_COLS;
    const int u = ex.bid() / ntiles, c0 = (ex.bid() % ntiles) * DFTP_COLS;
    if (u >= p.units) return;
    const int n1a = p.rowpair ? 2 * u : u, n1b = p.rowpair ? 2 * u + 1 : u;
    const size_t row_off = ((size_t)(u / p.ilv) * p.pitch) * p.ilv + u % p.ilv;
    const float sgn_im = p.inverse ? -1.f : 1.f;
    ex.each(st, [&](int tid, EmptyState&) {
        for (int j = tid; j < p.p; j += nt) { cf2 w = p.tw[(size_t)j * p.M]; w.y *= sgn_im; wp[j] = w; }
        for (int idx = tid; idx < p.p * DFTP_COLS; idx += nt) {
            const int s = idx / DFTP_COLS, c = c0 + idx % DFTP_COLS;
            cf4 v = {0.f, 0.f, 0.f, 0.f};
            if (c < p.ncols) {
                v = p.buf[(size_t)s * p.slice_stride + row_off + (size_t)c * p.ilv];
                if (p.inverse) {                   // conjugate twiddle first: slice index s is k2
                    cf2 wa = p.tw[(size_t)n1a * s], wb = p.tw[(size_t)n1b * s];
                    wa.y = -wa.y; wb.y = -wb.y;
                    const cf2 a = cmul({v.x, v.y}, wa), b = cmul({v.z, v.w}, wb);
                    v = {a.x, a.y, b.x, b.y};
                }
            }
            tile[idx] = v;
        }
    });
    ex.sync();
    // a thread owns one column and the outputs k = kl + j * (nt / 16): DFTP_KB of them share every tile
    // value it reads, and the two complex halves of a cf4 ride the packed-f32 ALU ops side by side
    ex.each(st, [&](int tid, EmptyState&) {
        const int cl = tid % DFTP_COLS, kl = tid / DFTP_COLS, kstep = nt / DFTP_COLS;
        const int c = c0 + cl;
        if (c >= p.ncols) return;
        for (int kb0 = kl; kb0 < p.p; kb0 += kstep * DFTP_KB) {
            vf2 accr[DFTP_KB], acci[DFTP_KB];
            int kk[DFTP_KB], wi[DFTP_KB];
#pragma unroll
            for (int j = 0; j < DFTP_KB; ++j) {
                const int k = kb0 + j * kstep;
                kk[j] = k < p.p ? k : 0;                 // (a lane past the end computes output 0 again and drops it)
                wi[j] = 0; accr[j] = mk2(0.f, 0.f); acci[j] = mk2(0.f, 0.f);
            }
            for (int sidx = 0; sidx < p.p; ++sidx) {
                const cf4 v = tile[sidx * DFTP_COLS + cl];
                const vf2 vr = mk2(v.x, v.z), vi = mk2(v.y, v.w);
#pragma unroll
                for (int j = 0; j < DFTP_KB; ++j) {
                    const cf2 w = wp[wi[j]];
                    accr[j] += vr * w.x - vi * w.y;
                    acci[j] += vr * w.y + vi * w.x;
                    wi[j] += kk[j]; if (wi[j] >= p.p) wi[j] -= p.p;
                }
            }
#pragma unroll
            for (int j = 0; j < DFTP_KB; ++j) {
                const int k = kb0 + j * kstep;
                if (k >= p.p) continue;
                cf2 a = {accr[j].x, acci[j].x}, b = {accr[j].y, acci[j].y};
                if (!p.inverse) {                  // slice index k is k2
                    a = cmul(a, p.tw[(size_t)n1a * k]); b = cmul(b, p.tw[(size_t)n1b * k]);
                }
                cf4 o = {a.x, a.y, b.x, b.y};
                p.buf[(size_t)k * p.slice_stride + row_off + (size_t)c * p.ilv] = o;
            }
        }
    });
}

// The same transform for p <= DFTP_PAIR_MAX_P with half the multiplies and no index arithmetic in the inner
// loop (the generic kernel spends more instructions on (s k) mod p than on the sums).  Outputs k and
// p - k use conjugate twiddles (c, -+s): with A = sum vr c, B = sum vi s, C = sum vr s, D = sum vi c
//     X[k] = (A - B, C + D),   X[p - k] = (A + B, D - C)
// so a "pair unit" h = 0 .. p/2 costs four (packed) FMAs per input for two outputs.  The matrix
// Wh[s][h] = W_p^(s h) sits in LDS, filled once per work-group, which then walks DFTP_UNITS row units.
constexpr int DFTP_PAIR_MAX_P = 126;
constexpr int DFTP_UNITS = 4;
SM_HD int dftp_pairs_cols(int p) {                 // columns per 256-thread work-group
    const int H = p / 2 + 1;
    if (H > 8) return DFTP_COLS;
    int h2 = 1;
    while (h2 < H) h2 *= 2;
    return 256 / h2 > 128 ? 128 : 256 / h2;
}
SM_HD size_t dftp_pairs_lds_bytes(int p) {
    const int H = p / 2 + 1;
    return (size_t)p * dftp_pairs_cols(p) * sizeof(cf4) + (size_t)p * H * sizeof(cf2);
}
template <int NP, class Ex, class St>
SM_HD void dftp_pairs_compute(Ex& ex, St& st, const DftpParams& p, const cf4* tile, const cf2* wh, int H, int c0,
                              size_t row_off, int n1a, int n1b) {
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        const int cl = tid % p.cols, hl = tid / p.cols, hstep = nt / p.cols;
        const int c = c0 + cl;
        if (c >= p.ncols) return;
        vf2 A[NP], B[NP], C[NP], D[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) { A[j] = mk2(0.f, 0.f); B[j] = A[j]; C[j] = A[j]; D[j] = A[j]; }
        const cf4* tp = tile + cl;
        const cf2* wq = wh + hl;                   // unit h = hl + j * hstep (reads past H land in the padding row)
        for (int sidx = 0; sidx < p.p; ++sidx) {
            const cf4 v = *tp;
            const vf2 vr = mk2(v.x, v.z), vi = mk2(v.y, v.w);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const cf2 w = wq[j * hstep];
                A[j] += vr * w.x; B[j] += vi * w.y; C[j] += vr * w.y; D[j] += vi * w.x;
            }
            tp += p.cols; wq += H;
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int h = hl + j * hstep;
            if (h >= H) continue;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int k = side == 0 ? h : p.p - h;
                if (side == 1 && (h == 0 || 2 * h == p.p)) continue;          // its own partner
                const vf2 re = side == 0 ? A[j] - B[j] : A[j] + B[j];
                const vf2 im = side == 0 ? C[j] + D[j] : D[j] - C[j];
                cf2 a = {re.x, im.x}, b = {re.y, im.y};
                if (!p.inverse) { a = cmul(a, p.tw[(size_t)n1a * k]); b = cmul(b, p.tw[(size_t)n1b * k]); }
                cf4 o = {a.x, a.y, b.x, b.y};
                p.buf[(size_t)k * p.slice_stride + row_off + (size_t)c * p.ilv] = o;
            }
        }
    });
}
template <class Ex>
SM_HD void k_dftp_pairs(Ex& ex, const DftpParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    const int H = p.p / 2 + 1;
    const int cols = p.cols;
    cf4* tile = (cf4*)(ex.lds() + LDS_SCRATCH_FLOATS);             // [p][cols]
    cf2* wh = (cf2*)(tile + (size_t)p.p * cols);                    // [p][H] (+ slack: the launch adds a row)
    const int ntiles = (p.ncols + cols - 1) / cols;
    const int ug = ex.bid() / ntiles, c0 = (ex.bid() % ntiles) * cols;
    const float sgn_im = p.inverse ? -1.f : 1.f;
    ex.each(st, [&](int tid, EmptyState&) {
        for (int idx = tid; idx < p.p * H; idx += nt) {
            const int sidx = idx / H, h = idx % H;
            cf2 w = p.tw[(size_t)((sidx * h) % p.p) * p.M];
            w.y *= sgn_im;
            wh[idx] = w;
        }
        for (int idx = p.p * H + tid; idx < (p.p + 1) * H + 64; idx += nt) { cf2 z = {0.f, 0.f}; wh[idx] = z; }
    });
    for (int uu = 0; uu < DFTP_UNITS; ++uu) {
        const int u = ug * DFTP_UNITS + uu;
        if (u >= p.units) break;
        const int n1a = p.rowpair ? 2 * u : u, n1b = p.rowpair ? 2 * u + 1 : u;
        const size_t row_off = ((size_t)(u / p.ilv) * p.pitch) * p.ilv + u % p.ilv;
        ex.sync();                                   // the previous unit's tile has been consumed (and wh is filled)
        ex.each(st, [&](int tid, EmptyState&) {
            for (int idx = tid; idx < p.p * cols; idx += nt) {
                const int sidx = idx / cols, c = c0 + idx % cols;
                cf4 v = {0.f, 0.f, 0.f, 0.f};
                if (c < p.ncols) {
                    v = p.buf[(size_t)sidx * p.slice_stride + row_off + (size_t)c * p.ilv];
                    if (p.inverse) {
                        cf2 wa = p.tw[(size_t)n1a * sidx], wb = p.tw[(size_t)n1b * sidx];
                        wa.y = -wa.y; wb.y = -wb.y;
                        const cf2 a = cmul({v.x, v.y}, wa), b = cmul({v.z, v.w}, wb);
                        v = {a.x, a.y, b.x, b.y};
                    }
                }
                tile[idx] = v;
            }
        });
        ex.sync();
        const int np = (H + nt / cols - 1) / (nt / cols);
        if (np <= 1) dftp_pairs_compute<1>(ex, st, p, tile, wh, H, c0, row_off, n1a, n1b);
        else if (np == 2) dftp_pairs_compute<2>(ex, st, p, tile, wh, H, c0, row_off, n1a, n1b);
        else if (np == 3) dftp_pairs_compute<3>(ex, st, p, tile, wh, H, c0, row_off, n1a, n1b);
        else dftp_pairs_compute<4>(ex, st, p, tile, wh, H, c0, row_off, n1a, n1b);
    }
}

// [R][C] -> [C][R], elements of 2 or 4 bytes moved as bits (64 x 64 tiles through LDS): a tensor
// whose ROW length is the rough one is merged transposed (fft2 commutes with the transpose and
// every statistic of the merge is a sum or an order statistic over all bins)
constexpr int TR_TILE = 64;         // 64 two-byte elements = one 128-byte line per tile row, both ways
struct TransposeParams { const void* src; void* dst; int R, C; int esize; };
template <class Ex>
SM_HD void k_transpose(Ex& ex, const TransposeParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int nt = ex.nthreads();
    uint32_t* tile = (uint32_t*)(ex.lds() + LDS_SCRATCH_FLOATS);   // [TR_TILE][TR_TILE + 1]
    const int tc = (p.C + TR_TILE - 1) / TR_TILE;
    const int r0 = (ex.bid() / tc) * TR_TILE, c0 = (ex.bid() % tc) * TR_TILE;
    ex.each(st, [&](int tid, EmptyState&) {
        for (int idx = tid; idx < TR_TILE * TR_TILE; idx += nt) {
            const int r = r0 + idx / TR_TILE, c = c0 + idx % TR_TILE;
            uint32_t v = 0;
            if (r < p.R && c < p.C) {
                const size_t i = (size_t)r * p.C + c;
                v = p.esize == 4 ? ((const uint32_t*)p.src)[i] : (uint32_t)((const uint16_t*)p.src)[i];
            }
            tile[(idx / TR_TILE) * (TR_TILE + 1) + idx % TR_TILE] = v;
        }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int idx = tid; idx < TR_TILE * TR_TILE; idx += nt) {
            const int c = c0 + idx / TR_TILE, r = r0 + idx % TR_TILE;
            if (r < p.R && c < p.C) {
                const uint32_t v = tile[(idx % TR_TILE) * (TR_TILE + 1) + idx / TR_TILE];
                const size_t o = (size_t)c * p.R + r;
                if (p.esize == 4) ((uint32_t*)p.dst)[o] = v; else ((uint16_t*)p.dst)[o] = (uint16_t)v;
            }
        }
    });
}

// ---- kernel tags (sm_tag.hpp) ----
SM_KERNEL_TAG(KDeltaNorms, DeltaNormsParams, "delta_norms", k_delta_norms(ex, p))
SM_KERNEL_TAG(KSumPartialsN, SumNParams, "sum_partials", k_sum_partials_n(ex, p))
SM_KERNEL_TAG(KBlend, BlendParams, "blend", k_blend(ex, p))
SM_KERNEL_TAG(KCombine, CombineParams, "combine", k_combine(ex, p))
SM_KERNEL_TAG(KExpand, ExpandParams, "expand_full", k_expand(ex, p))
SM_KERNEL_TAG(KPack, PackParams, "pack_planes", k_pack(ex, p))
SM_KERNEL_TAG(KSplit, SplitParams, "split_complex", k_split(ex, p))
SM_KERNEL_TAG(KJoin, JoinParams, "join_complex", k_join(ex, p))
SM_KERNEL_TAG(KCull, CullParams, "cull_inplace", k_cull(ex, p))
SM_KERNEL_TAG(KAddition, AdditionParams, "addition_merge", k_addition(ex, p))
SM_KERNEL_TAG(KFnSums, FnSumsParams, "fn_slerp_sums", k_fn_sums(ex, p))
SM_KERNEL_TAG(KFnSlerpFin, FnSlerpFinParams, "fn_slerp_consts", k_fn_slerp_fin(ex, p))
SM_KERNEL_TAG(KFnSlerpRows0, FnSlerpRowsParams, "fn_slerp_relnorm", k_fn_slerp_rows<0>(ex, p))
SM_KERNEL_TAG(KFnSlerpRows1, FnSlerpRowsParams, "fn_slerp_out", k_fn_slerp_rows<1>(ex, p))
SM_KERNEL_TAG(KFnSlerpDen, FnSlerpDenParams, "fn_slerp_den", k_fn_slerp_den(ex, p))
SM_KERNEL_TAG(KSumsqAny, SumsqAnyParams, "fn_sumsq", k_sumsq_any(ex, p))
SM_KERNEL_TAG(KDivScalar, DivScalarParams, "fn_div_scalar", k_div_scalar(ex, p))
SM_KERNEL_TAG(KCorrPartial, CorrPartialParams, "correlate_pairs", k_corr_partial(ex, p))
SM_KERNEL_TAG(KCorrFinish, CorrFinishParams, "correlate_finish", k_corr_finish(ex, p))
SM_KERNEL_TAG(KSerialNorm, SerialNormParams, "serial_norm", k_serial_norm(ex, p))
SM_KERNEL_TAG(KSpecNorm, SpecNormParams, "spec_norm", k_spec_norm(ex, p))
SM_KERNEL_TAG(KSumsqCand, SumsqCandParams, "spec_norm_cand", k_sumsq_cand(ex, p))
SM_KERNEL_TAG(KSumSpec, SumSpecParams, "spec_norm_sum", k_sum_spec(ex, p))
SM_KERNEL_TAG(KSpecRescale, SpecRescaleParams, "spec_rescale", k_spec_rescale(ex, p))
SM_KERNEL_TAG(KDftp, DftpParams, "dft_across_slices", k_dftp(ex, p))
SM_KERNEL_TAG(KDftpPairs, DftpParams, "dft_across_slices", k_dftp_pairs(ex, p))
SM_KERNEL_TAG(KTranspose, TransposeParams, "transpose", k_transpose(ex, p))
// this header's share of group 2 of smhip_side.hip (smhip_device.hpp)
#define SM_KERNELS_MERGE(X) X(KDeltaNorms) X(KSumPartialsN) X(KBlend) X(KCombine) X(KExpand) X(KPack) X(KSplit) X(KJoin) \
    X(KCull) X(KAddition) X(KFnSums) X(KFnSlerpFin) X(KFnSlerpRows0) X(KFnSlerpRows1) X(KFnSlerpDen) X(KSumsqAny) X(KDivScalar) \
    X(KCorrPartial) X(KCorrFinish) X(KSerialNorm) X(KSpecNorm) X(KSumsqCand) X(KSumSpec) X(KSpecRescale) X(KDftp) X(KDftpPairs) X(KTranspose)

}  // namespace smhip
