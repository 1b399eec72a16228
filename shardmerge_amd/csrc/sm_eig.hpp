// sm_eig.hpp - the device-side symmetric eigensolver (smhip_sym_eig_par): a parallel-ordered Jacobi iteration on a batch
// of small dense symmetric fp64 matrices, one work-group per matrix and the whole iteration in ONE launch.  The function
// is stated step by step in include/shardmerge_hip.h; every value below is defined bit for bit, one rounded fp64
// operation at a time (geo_dadd / geo_dmul / geo_ddiv / geo_dsqrt), so the gfx950 build, the g++ emulator and a numpy
// restatement agree.
//
//   The ordering is a round-robin tournament (Brent and Luk) on m = n rounded up to even: a sweep is m - 1 rounds, a
//   round is m / 2 disjoint pairs, "slot" i of round r holds {m-1, r} (i = 0) or {(r + i) mod (m-1), (r - i) mod (m-1)}.
//   A round has two phases with a work-group barrier after each:
//     1. slot i's thread computes (c, s, t, rotated) of its pair from the matrix as it stands into a table in LDS.
//     2. the update A <- J^T A J, J the product of the round's rotations.  The work item is the 2 x 2 block that the
//        slots i <= j cut out of A: a thread reads its four values, applies the row side (slot i's rotation), then the
//        column side (slot j's) and writes the result to both triangles; the diagonal block i == j takes the closed form
//        of the cyclic solver.  The blocks of a round are disjoint, so the update is in place.  In the same phase the
//        columns p, q of V of every rotated pair are updated, one thread per row and pair.
//   The h (h + 1) / 2 blocks, h = m / 2, are numbered without a search: with g = the odd one of h, h + 1, an item is
//   (a, b), a < g, and stands for the unordered pair {a, (a + b) mod g}; for odd h that is block {a, a'} itself (b = 0: the
//   diagonal), for even h the pairs x < y of g = h + 1 elements are the blocks (x, y - 1).
//
//   Where A and V live (chosen on the host from n; gfx950 has 160 KiB of LDS):
//     plan 1  n <= 96    both in LDS
//     plan 2  n <= 128   A in LDS, V in the caller's workspace
//     plan 3  n <= 272   both in the workspace, which the one work-group walks (578 KiB at n = 272: it stays in L2)
//   The row pitch of A and V is m + 1 doubles, an ODD number: a wave's lanes hold one slot i and consecutive slots j, so
//   the reads A[p_i][p_j] run along a row (consecutive banks) while the mirrored writes A[p_j][p_i] run down a column; with
//   an even pitch (80 doubles = 160 words) those land in two of the 64 banks, with an odd pitch 32 consecutive rows cover
//   all 64 banks once.
#pragma once
#include "sm_extract.hpp"

namespace smhip {

constexpr int EIG_PLAN1_MAX_N = 96;
constexpr int EIG_PLAN2_MAX_N = 128;
constexpr int EIG_MAX_THREADS = 1024;

SM_HD int eig_even(int n) { return (n + 1) & ~1; }
SM_HD int eig_pitch(int n) { return eig_even(n) + 1; }
SM_HD int eig_plan(int n) { return n <= EIG_PLAN1_MAX_N ? 1 : (n <= EIG_PLAN2_MAX_N ? 2 : 3); }
SM_HD int eig_blocks(int n) { const int h = eig_even(n) / 2; return h * (h + 1) / 2; }
// the table of a round at the start of LDS: thr, the sweep that last rotated and the non-finite flag (ints), then per
// slot c, s, t (doubles) and p, q, rotated (ints); rounded up to 16 bytes
SM_HD size_t eig_table_bytes(int n) {
    const size_t h = (size_t)eig_even(n) / 2;
    return (16 + h * (3 * 8 + 3 * 4) + 15) / 16 * 16;
}
SM_HD size_t eig_lds_bytes(int n) {
    const size_t mat = (size_t)n * eig_pitch(n) * 8;
    const int plan = eig_plan(n);
    return eig_table_bytes(n) + (plan == 1 ? 2 * mat : (plan == 2 ? mat : 0));
}
// the workspace of one matrix, in doubles: V [n][pitch] | the diagonal [n] | sweeps (an int in 8 bytes) | A [n][pitch] (plan 3)
SM_HD size_t eig_ws_doubles(int n) {
    const size_t mat = (size_t)n * eig_pitch(n);
    return mat + n + 1 + (eig_plan(n) == 3 ? mat : 0);
}
SM_HD int eig_threads(int n) {
    const int b = (eig_blocks(n) + 63) / 64 * 64;
    return b > EIG_MAX_THREADS ? EIG_MAX_THREADS : b;
}

struct EigJacobiParams {
    const double* a;            // [batch][n][lda], both triangles; not written
    double* ws;                 // [batch][eig_ws_doubles(n)]
    int n, lda;
};

template <class Ex>
SM_HD void k_eig_jacobi(Ex& ex, const EigJacobiParams& p) {
    typename Ex::template State<EmptyState> st;
    ex.init(st);
    const int n = p.n, m = eig_even(n), h = m / 2, pitch = eig_pitch(n), plan = eig_plan(n);
    const size_t mat = (size_t)n * pitch;
    const double* src = p.a + (size_t)ex.bid() * n * p.lda;
    double* ws = p.ws + (size_t)ex.bid() * eig_ws_doubles(n);
    char* lds = (char*)ex.lds();
    double* thr_p = (double*)lds;
    volatile int* last_rot = (volatile int*)(lds + 8);
    volatile int* bad = (volatile int*)(lds + 12);              // an entry of the input is a NaN or an Inf
    double* tc = (double*)(lds + 16);
    double* ts = tc + h;
    double* tt = ts + h;
    int* tp = (int*)(tt + h);
    int* tq = tp + h;
    int* trot = tq + h;
    double* lmat = (double*)(lds + eig_table_bytes(n));
    double* A = plan == 3 ? ws + mat + n + 1 : lmat;
    double* V = plan == 1 ? lmat + mat : ws;
    double* diag = ws + mat;
    const int nthr = ex.nthreads();

    ex.each(st, [&](int tid, EmptyState&) {
        if (tid == 0) { *last_rot = 0; *bad = 0; }
    });
    ex.sync();
    ex.each(st, [&](int tid, EmptyState&) {
        for (int e = tid; e < n * n; e += nthr) {
            const int i = e / n, j = e % n;
            const double x = src[(size_t)i * p.lda + j];
            if (!geo_finite(x)) *bad = 1;
            A[(size_t)i * pitch + j] = x;
            V[(size_t)i * pitch + j] = i == j ? 1.0 : 0.0;
        }
        if (tid == 0) {
            double scale = 0.0;
            for (int i = 0; i < n; ++i) scale = geo_dadd(scale, fabs(src[(size_t)i * p.lda + i]));
            *thr_p = geo_dmul(scale, 0x1p-70);
        }
    });
    ex.sync();
    // (finiteness is the caller's check; a matrix that fails it is not iterated on and reports sweeps = -1)
    const int rounds = *bad ? 0 : XL_EIG_SWEEPS * (m - 1);

    const int g = (h & 1) ? h : h + 1, half = (g - 1) / 2;
    const int bw = (h & 1) ? half + 1 : half;                   // items per a
    const int nblk = g * bw, nvit = n * h;
    int sweeps = 0;
    for (int round = 0; round < rounds; ++round) {
        const int r = round % (m - 1), sweep = round / (m - 1) + 1;
        // phase 1: the round's pairs and their rotations, from the matrix as it stands
        ex.each(st, [&](int tid, EmptyState&) {
            for (int i = tid; i < h; i += nthr) {
                int x = m - 1, y = r;
                if (i) { x = (r + i) % (m - 1); y = (r - i + m - 1) % (m - 1); }
                const int pp = x < y ? x : y, qq = x < y ? y : x;
                tp[i] = pp; tq[i] = qq;
                int rot = 0;
                if (qq < n) {                                   // (else the bye)
                    const double apq = A[(size_t)pp * pitch + qq];
                    if (fabs(apq) > *thr_p) {
                        rot = 1;
                        const double app = A[(size_t)pp * pitch + pp], aqq = A[(size_t)qq * pitch + qq];
                        const double theta = geo_ddiv(geo_dadd(aqq, -app), geo_dmul(2.0, apq));
                        const double den = geo_dadd(fabs(theta), geo_dsqrt(geo_dadd(geo_dmul(theta, theta), 1.0)));
                        const double t = geo_ddiv(theta < 0.0 ? -1.0 : 1.0, den);
                        const double c = geo_ddiv(1.0, geo_dsqrt(geo_dadd(geo_dmul(t, t), 1.0)));
                        tc[i] = c; ts[i] = geo_dmul(t, c); tt[i] = t;
                        *last_rot = sweep;
                    }
                }
                trot[i] = rot;
            }
        });
        ex.sync();
        // phase 2: the blocks i <= j, and the columns of V
        ex.each(st, [&](int tid, EmptyState&) {
            for (int w = tid; w < nblk; w += nthr) {
                const int a = w / bw, b = w % bw + ((h & 1) ? 0 : 1);
                int a2 = a + b;
                if (a2 >= g) a2 -= g;
                int i = a < a2 ? a : a2, j = a < a2 ? a2 : a;
                if (!(h & 1)) --j;
                const int ri = trot[i], rj = trot[j];
                if (!(ri | rj)) continue;
                const int pi = tp[i], qi = tq[i];
                if (i == j) {
                    double* app = A + (size_t)pi * pitch + pi;
                    double* aqq = A + (size_t)qi * pitch + qi;
                    const double tap = geo_dmul(tt[i], A[(size_t)pi * pitch + qi]);
                    *app = geo_dadd(*app, -tap);
                    *aqq = geo_dadd(*aqq, tap);
                    A[(size_t)pi * pitch + qi] = 0.0; A[(size_t)qi * pitch + pi] = 0.0;
                    continue;
                }
                const int pj = tp[j], qj = tq[j];
                if (qi >= n) {
                    // the bye (always slot 0, so always the row slot) holds one live index, its p: the block is the
                    // 1 x 2 strip of row p, which takes the column side alone
                    const double c = tc[j], s = ts[j];
                    const double yp = A[(size_t)pi * pitch + pj], yq = A[(size_t)pi * pitch + qj];
                    const double zp = geo_dadd(geo_dmul(c, yp), -geo_dmul(s, yq));
                    const double zq = geo_dadd(geo_dmul(s, yp), geo_dmul(c, yq));
                    A[(size_t)pi * pitch + pj] = zp; A[(size_t)pj * pitch + pi] = zp;
                    A[(size_t)pi * pitch + qj] = zq; A[(size_t)qj * pitch + pi] = zq;
                    continue;
                }
                double xpp = A[(size_t)pi * pitch + pj], xpq = A[(size_t)pi * pitch + qj];
                double xqp = A[(size_t)qi * pitch + pj], xqq = A[(size_t)qi * pitch + qj];
                if (ri) {                                       // Y = R_P^T X
                    const double c = tc[i], s = ts[i];
                    const double ypp = geo_dadd(geo_dmul(c, xpp), -geo_dmul(s, xqp));
                    const double yqp = geo_dadd(geo_dmul(s, xpp), geo_dmul(c, xqp));
                    const double ypq = geo_dadd(geo_dmul(c, xpq), -geo_dmul(s, xqq));
                    const double yqq = geo_dadd(geo_dmul(s, xpq), geo_dmul(c, xqq));
                    xpp = ypp; xqp = yqp; xpq = ypq; xqq = yqq;
                }
                if (rj) {                                       // Z = Y R_Q
                    const double c = tc[j], s = ts[j];
                    const double zpp = geo_dadd(geo_dmul(c, xpp), -geo_dmul(s, xpq));
                    const double zpq = geo_dadd(geo_dmul(s, xpp), geo_dmul(c, xpq));
                    const double zqp = geo_dadd(geo_dmul(c, xqp), -geo_dmul(s, xqq));
                    const double zqq = geo_dadd(geo_dmul(s, xqp), geo_dmul(c, xqq));
                    xpp = zpp; xpq = zpq; xqp = zqp; xqq = zqq;
                }
                A[(size_t)pi * pitch + pj] = xpp; A[(size_t)pj * pitch + pi] = xpp;
                A[(size_t)pi * pitch + qj] = xpq; A[(size_t)qj * pitch + pi] = xpq;
                A[(size_t)qi * pitch + pj] = xqp; A[(size_t)pj * pitch + qi] = xqp;
                A[(size_t)qi * pitch + qj] = xqq; A[(size_t)qj * pitch + qi] = xqq;
            }
            for (int w = tid; w < nvit; w += nthr) {
                const int k = w / h, i = w % h;
                if (!trot[i]) continue;
                double* vp = V + (size_t)k * pitch + tp[i];
                double* vq = V + (size_t)k * pitch + tq[i];
                const double c = tc[i], s = ts[i], a = *vp, b = *vq;
                *vp = geo_dadd(geo_dmul(c, a), -geo_dmul(s, b));
                *vq = geo_dadd(geo_dmul(s, a), geo_dmul(c, b));
            }
        });
        ex.sync();
        if (r == m - 2) {
            sweeps = sweep;
            const int last = *last_rot;
            ex.sync();                                          // every thread has read it before the next sweep writes it
            if (last != sweep) break;
        }
    }

    // the diagonal, V (plan 1: out of LDS) and the sweeps run; sort and signs are the host's (xl_eig_sort_signs)
    ex.each(st, [&](int tid, EmptyState&) {
        for (int i = tid; i < n; i += nthr) diag[i] = A[(size_t)i * pitch + i];
        if (plan == 1)
            for (int e = tid; e < n * n; e += nthr) ws[(size_t)(e / n) * pitch + e % n] = V[(size_t)(e / n) * pitch + e % n];
        if (tid == 0) *(int*)(diag + n) = rounds ? sweeps : -1;
    });
}

// ---- kernel tag (sm_tag.hpp) and group 23 of smhip_side.hip (smhip_device.hpp) ----
// one work-group of up to 1024 threads per matrix; a thread holds one 2 x 2 block and two rotations: far below 128 VGPRs
SM_KERNEL_TAG_LB(KEigJacobi, EigJacobiParams, "eig_jacobi", k_eig_jacobi(ex, p), 1024, 4)
#define SM_SIDE_KERNELS_23(X) X(KEigJacobi)

}  // namespace smhip
