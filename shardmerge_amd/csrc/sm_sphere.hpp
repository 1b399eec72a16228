// sm_sphere.hpp - the Karcher-mean merges (karcher, multislerp): the weighted mean ON THE SPHERE of the directions of k
// vectors, their lengths averaged linearly.  The function is stated in include/shardmerge_hip.h (smhip_sphere_merge).
// The mean of k unit vectors lies in their span, so the iteration never touches the tensors: it runs on k coefficients
// against the k x k Gram that geo_gram (sm_geo.hpp) already produces in ordered fp64, and geo_combine writes the result.
//
//   sm_acos / sm_sin / sm_cos   the trigonometry, DEFINED here instead of borrowed from a library: Horner evaluations of
//                  truncated Taylor series over geo_dadd / geo_dmul / geo_ddiv / geo_dsqrt, one rounded fp64 operation at
//                  a time, so the host, the device, the CPU emulator and a numpy restatement give the same bits.
//   sphere_coefficients   step 3 of the definition, shared by the host (whole tensor) and the device (per row).
//   sphere_coef    row-wise: a thread per row turns its Gram into the k coefficients, an iteration count and flags.
//                  k <= 4: every array in registers (the loops are unrolled, every index a constant); larger k: the
//                  thread's H, a, t and w in LDS, [slot][thread], and a work-group as large as 96 KiB of them allow.
//   sphere_fn      the probe behind smhip_sphere_fn: y[i] = sm_acos / sm_sin / sm_cos (x[i]).
#pragma once
#include "sm_geo.hpp"

namespace smhip {

constexpr double SPH_PI = 0x1.921fb54442d18p+1, SPH_PIO2 = 0x1.921fb54442d18p+0;       // fp64(pi), fp64(pi / 2)
constexpr double SPH_SMALL = 1e-8;                // below it theta / sin(theta) and sin(tau) / tau are 1
constexpr double SPH_QMIN = 1e-16;                // a^T H a at or below it: the unit vectors cancel
enum { SPH_ACOS = 0, SPH_SIN = 1, SPH_COS = 2 };
enum { SPH_CONVERGED = 1, SPH_LINEAR = 2 };       // a row's flags

// p = c[N-1]; p = p * z + c[i] for i = N-2 .. 0: two rounded operations per step
template <int N>
SM_HD double sph_horner(const double (&c)[N], double z) {
    double p = c[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) p = geo_dadd(geo_dmul(p, z), c[i]);
    return p;
}

// asin(z) = z * P(z^2) for |z| <= 1/2: the Taylor series sum_m (2m)! / (4^m (m!)^2 (2m + 1)) z^(2m+1), m = 0..23 (degree
// 47; the first term left out is below 2^-57 at z = 1/2).  The coefficients are the exact rationals rounded to fp64.
SM_HD double sph_asin_half(double z) {
    const double c[24] = {
        0x1.0000000000000p+0, 0x1.5555555555555p-3, 0x1.3333333333333p-4, 0x1.6db6db6db6db7p-5,
        0x1.f1c71c71c71c7p-6, 0x1.6e8ba2e8ba2e9p-6, 0x1.1c4ec4ec4ec4fp-6, 0x1.c99999999999ap-7,
        0x1.7a87878787878p-7, 0x1.3fde50d79435ep-7, 0x1.12ef3cf3cf3cfp-7, 0x1.df3bd37a6f4dfp-8,
        0x1.a6863d70a3d71p-8, 0x1.782dda12f684cp-8, 0x1.51ba308d3dcb1p-8, 0x1.31683bdef7bdfp-8,
        0x1.15ee9d45d1746p-8, 0x1.fcaf8fb6db6dbp-9, 0x1.d3d2a8e0dd67dp-9, 0x1.b026f57b13b14p-9,
        0x1.90cb77f60c7cep-9, 0x1.750de64d7d05fp-9, 0x1.5c5f56efaaaabp-9, 0x1.464c0950f7d47p-9};
    return geo_dmul(z, sph_horner(c, geo_dmul(z, z)));
}
// acos on [-1, 1].  |x| <= 1/2: pi/2 - asin(x).  x > 1/2: 2 asin(sqrt((1 - x) / 2)) (1 - x and the halving are exact).
// x < -1/2: pi - 2 asin(sqrt((1 + x) / 2)).  acos(1) = +0 and acos(-1) = fp64(pi) exactly; a NaN gives a NaN.
SM_HD double sm_acos(double x) {
    if (x > 0.5) return geo_dmul(2.0, sph_asin_half(geo_dsqrt(geo_dmul(geo_dadd(1.0, -x), 0.5))));
    if (x < -0.5) return geo_dadd(SPH_PI, -geo_dmul(2.0, sph_asin_half(geo_dsqrt(geo_dmul(geo_dadd(1.0, x), 0.5)))));
    return geo_dadd(SPH_PIO2, -sph_asin_half(x));
}
// sin and cos on [0, pi]: x > pi/2 is reflected to y = pi - x (sin(x) = sin(y), cos(x) = -cos(y)), then the Taylor series
// in y^2 on [0, pi/2]: sin(y) = y * S(y^2), 12 terms (degree 23), cos(y) = C(y^2), 13 terms (degree 24); the first term
// left out is below 2^-59 at pi/2.  The coefficients are +-1 / n! rounded to fp64.
SM_HD double sm_sin(double x) {
    const double c[12] = {
        0x1.0000000000000p+0, -0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13,
        0x1.71de3a556c734p-19, -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41,
        0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57, 0x1.71b8ef6dcf572p-66, -0x1.761b41316381ap-75};
    const double y = x > SPH_PIO2 ? geo_dadd(SPH_PI, -x) : x;
    return geo_dmul(y, sph_horner(c, geo_dmul(y, y)));
}
SM_HD double sm_cos(double x) {
    const double c[13] = {
        0x1.0000000000000p+0, -0x1.0000000000000p-1, 0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10,
        0x1.a01a01a01a01ap-16, -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37,
        0x1.ae7f3e733b81fp-45, -0x1.6827863b97d97p-53, 0x1.e542ba4020225p-62, -0x1.0ce396db7f853p-70,
        0x1.f2cf01972f578p-80};
    const bool up = x > SPH_PIO2;
    const double y = up ? geo_dadd(SPH_PI, -x) : x;
    const double v = sph_horner(c, geo_dmul(y, y));
    return up ? -v : v;
}
SM_HD double sphere_fn(int op, double x) { return op == SPH_ACOS ? sm_acos(x) : (op == SPH_SIN ? sm_sin(x) : sm_cos(x)); }

// ---- where a row's H (packed upper triangle with its diagonal), a, t and w live -------------------------------------
// registers (or the host's stack): KM bounds k at compile time
template <int KM>
struct SphereRegs {
    double h[KM * (KM + 1) / 2], av[KM], tv[KM], wv[KM];
    SM_HD double& H(int i, int j) { return h[i <= j ? geo_pair_index(i, j, KM) : geo_pair_index(j, i, KM)]; }
    SM_HD double& a(int i) { return av[i]; }
    SM_HD double& t(int i) { return tv[i]; }
    SM_HD double& w(int i) { return wv[i]; }
};
// LDS: slot s of thread tid at base[s * nt + tid]; geo_pairs(k) + 3 k slots
SM_HD int sphere_slots(int k) { return geo_pairs(k) + 3 * k; }
struct SphereLds {
    double* base;               // + tid
    int nt, k;
    SM_HD double& H(int i, int j) { return base[(size_t)(i <= j ? geo_pair_index(i, j, k) : geo_pair_index(j, i, k)) * nt]; }
    SM_HD double& a(int i) { return base[(size_t)(geo_pairs(k) + i) * nt]; }
    SM_HD double& t(int i) { return base[(size_t)(geo_pairs(k) + k + i) * nt]; }
    SM_HD double& w(int i) { return base[(size_t)(geo_pairs(k) + 2 * k + i) * nt]; }
};

// i = 0 .. k-1 in ascending order; UNROLL: KM copies of the body, each with a constant i
template <int KM, bool UNROLL, class F>
SM_HD void sph_for(int k, F&& f) {
    if constexpr (UNROLL) {
        static_for<0, KM>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if (i < k) f(i);
        });
    } else {
        for (int i = 0; i < k; ++i) f(i);
    }
}

struct SphereOut {
    int iterations;             // how often tau was evaluated
    int flags;                  // SPH_CONVERGED | SPH_LINEAR
    double tau;                 // the last tau evaluated, 0 when none was
    double N;                   // sum_i w_i n_i
};

// Step 3 of smhip_sphere_merge.  G: the packed Gram of k vectors; A: ((0 + alpha_0) + ...) > 0.  Leaves H, the final a
// and w in `s`, the coefficients in c[0 .. k-1].
template <int KM, bool UNROLL, class Store>
SM_HD void sphere_coefficients(Store& s, const double* G, const double* alpha, double A, int k, int max_iter, double tol,
                               float* c, SphereOut& o) {
    auto each = [&](auto&& f) { sph_for<KM, UNROLL>(k, f); };
    // v^T H v = sum_i v_i (sum_j H_ij v_j), both sums ascending from +0; sel 0: a, 1: t
    auto quad = [&](int sel) {
        double Q = 0.0;
        each([&](int i) {
            double r = 0.0;
            each([&](int j) { r = geo_dadd(r, geo_dmul(s.H(i, j), sel ? s.t(j) : s.a(j))); });
            Q = geo_dadd(Q, geo_dmul(sel ? s.t(i) : s.a(i), r));
        });
        return Q;
    };
    // the weights, renormalised over the active vectors (n_i > 0 and w_i > 0)
    double W = 0.0;
    int nact = 0;
    each([&](int i) {
        const double wi = geo_ddiv(alpha[i], A);
        const bool active = geo_dsqrt(G[geo_pair_index(i, i, k)]) > 0.0 && wi > 0.0;
        s.w(i) = active ? wi : 0.0;
        if (active) { W = geo_dadd(W, wi); ++nact; }
    });
    double N = 0.0;
    each([&](int i) {
        if (s.w(i) > 0.0) s.w(i) = geo_ddiv(s.w(i), W);
        N = geo_dadd(N, geo_dmul(s.w(i), geo_dsqrt(G[geo_pair_index(i, i, k)])));
        s.a(i) = s.w(i);
        s.t(i) = 0.0;
    });
    // the normalised Gram
    each([&](int i) {
        const double ni = geo_dsqrt(G[geo_pair_index(i, i, k)]);
        each([&](int j) {
            if (j == i) s.H(i, i) = 1.0;
            if (j > i) s.H(i, j) = geo_cos(G[geo_pair_index(i, j, k)], ni, geo_dsqrt(G[geo_pair_index(j, j, k)]));
        });
    });
    o.iterations = 0; o.flags = 0; o.tau = 0.0; o.N = N;
    bool linear = false;
    if (nact <= 1) {                                   // nothing to average: a = w is (0, ..), or one 1
        o.flags = SPH_CONVERGED;
        each([&](int i) { c[i] = (float)s.a(i); });
        return;
    }
    double q = quad(0);
    if (!(q > SPH_QMIN) || !geo_finite(q)) {
        linear = true;
    } else {
        const double r = geo_dsqrt(q);
        each([&](int i) { s.a(i) = geo_ddiv(s.a(i), r); });
    }
    for (int it = 0; it < max_iter && !linear; ++it) {
        o.iterations = it + 1;
        // the log map of every vector at the current point, in coefficients: t = sum_j w_j f_j (u_j - d_j m)
        double g = 0.0;
        each([&](int j) {
            double d = 0.0;
            each([&](int i) { d = geo_dadd(d, geo_dmul(s.a(i), s.H(i, j))); });
            d = d > 1.0 ? 1.0 : (d < -1.0 ? -1.0 : d);
            const double th = sm_acos(d);
            double f = 1.0;
            if (!(th < SPH_SMALL)) {
                const double sn = sm_sin(th);
                f = sn < SPH_SMALL ? 0.0 : geo_ddiv(th, sn);
            }
            const double p = geo_dmul(s.w(j), f);
            s.t(j) = p;
            g = geo_dadd(g, geo_dmul(p, d));
        });
        each([&](int i) { s.t(i) = geo_dadd(s.t(i), -geo_dmul(s.a(i), g)); });
        const double tau2 = quad(1);
        if (!geo_finite(tau2)) { linear = true; break; }
        double tau = geo_dsqrt(tau2 > 0.0 ? tau2 : 0.0);
        if (tau > SPH_PI) tau = SPH_PI;
        o.tau = tau;
        if (tau < tol) { o.flags = SPH_CONVERGED; break; }
        // the exponential map: a step of length tau along t
        const double cs = sm_cos(tau), sc = tau < SPH_SMALL ? 1.0 : geo_ddiv(sm_sin(tau), tau);
        each([&](int i) { s.a(i) = geo_dadd(geo_dmul(cs, s.a(i)), geo_dmul(sc, s.t(i))); });
        q = quad(0);
        if (!(q > SPH_QMIN) || !geo_finite(q)) { linear = true; break; }
        const double r = geo_dsqrt(q);
        each([&](int i) { s.a(i) = geo_ddiv(s.a(i), r); });
    }
    if (linear) {
        o.flags = SPH_LINEAR;
        each([&](int i) { c[i] = (float)s.w(i); });
        return;
    }
    each([&](int i) {
        c[i] = s.w(i) > 0.0 ? (float)geo_ddiv(geo_dmul(s.a(i), N), geo_dsqrt(G[geo_pair_index(i, i, k)])) : 0.f;
    });
}

// ---- sphere_coef: the row Grams of geo_gram -> [R][k] coefficients, iteration counts and flags ----------------------
constexpr int SPH_REG_SMALL = 4;                  // k <= 4: registers
constexpr int SPH_REG_THREADS = 256;
constexpr size_t SPH_LDS_BYTES = 96 * 1024;       // larger k: the budget of the threads' slots
// the work-group of the LDS instantiation: the largest of 256, 128, 64 whose slots fit (k <= 6, k <= 10, k <= 16)
SM_HD int sphere_coef_threads(int k) {
    if (k <= SPH_REG_SMALL) return SPH_REG_THREADS;
    for (int nt = 256; nt > 64; nt >>= 1)
        if ((size_t)sphere_slots(k) * 8 * nt <= SPH_LDS_BYTES) return nt;
    return 64;
}
SM_HD size_t sphere_coef_lds_floats(int k) {
    return LDS_SCRATCH_FLOATS + (k <= SPH_REG_SMALL ? 0 : (size_t)sphere_slots(k) * 2 * sphere_coef_threads(k));
}
struct SphereCoefParams {
    int k, max_iter;
    size_t rows;
    double tol;
    double alpha[TIES_MAX_MODELS];
    double A;                   // ((0 + alpha_0) + alpha_1) + ...
    const double* G;            // [rows][geo_pairs(k)]
    float* coef;                // [rows][k]
    int* iters;                 // [rows]
    int* flags;                 // [rows]: SPH_CONVERGED | SPH_LINEAR
};
template <bool LDS, class Ex>
SM_HD void k_sphere_coef(Ex& ex, const SphereCoefParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    double* slots = (double*)(ex.lds() + LDS_SCRATCH_FLOATS);       // (LDS_SCRATCH_FLOATS is even)
    const int nt = ex.nthreads();
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t r = (size_t)ex.bid() * nt + tid;
        if (r >= p.rows) return;
        const double* G = p.G + r * geo_pairs(p.k);
        float* c = p.coef + r * p.k;
        SphereOut o;
        if constexpr (LDS) {
            SphereLds s{slots + tid, nt, p.k};
            sphere_coefficients<TIES_MAX_MODELS, false>(s, G, p.alpha, p.A, p.k, p.max_iter, p.tol, c, o);
        } else {
            SphereRegs<SPH_REG_SMALL> s;
            sphere_coefficients<SPH_REG_SMALL, true>(s, G, p.alpha, p.A, p.k, p.max_iter, p.tol, c, o);
        }
        p.iters[r] = o.iterations;
        p.flags[r] = o.flags;
    });
}

struct SphereFnParams {
    int op;                     // SPH_ACOS / SPH_SIN / SPH_COS
    size_t n;
    const double* x;
    double* y;
};
template <class Ex>
SM_HD void k_sphere_fn(Ex& ex, const SphereFnParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    ex.each(st, [&](int tid, EmptyState&) {
        const size_t i = (size_t)ex.bid() * ex.nthreads() + tid;
        if (i < p.n) p.y[i] = sphere_fn(p.op, p.x[i]);
    });
}

// ---- kernel tags (sm_tag.hpp) and this header's share of group 7 of smhip_side.hip (smhip_device.hpp) ----
// the row-wise coefficient iteration, k <= 4 in registers or up to 16 in LDS, and the probe of the three defined functions
SM_KERNEL_TAG_LB(KSphereCoef, SphereCoefParams, "sphere_coef", k_sphere_coef<false>(ex, p), SPH_REG_THREADS, 2)
SM_KERNEL_TAG_LB(KSphereCoefLds, SphereCoefParams, "sphere_coef", k_sphere_coef<true>(ex, p), 256, 2)
SM_KERNEL_TAG_LB(KSphereFn, SphereFnParams, "sphere_fn", k_sphere_fn(ex, p), 256, 4)
#define SM_KERNELS_SPHERE(X) X(KSphereCoef) X(KSphereCoefLds) X(KSphereFn)

}  // namespace smhip
