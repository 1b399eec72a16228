"""numpy restatement of smhip_sym_eig_par (include/shardmerge_hip.h): the parallel-ordered Jacobi iteration, one rounded
fp64 operation at a time.  A round is vectorised over its disjoint pairs: with the row side applied to whole rows and then
the column side to whole columns, every element takes the row side first and the column side second; a skipped pair's
rows and columns are not touched.  That is the function's block Z for a pair P before a pair Q; the block of Q before P
is then written from it, as the function states."""
import numpy as np

EIG_SWEEPS = 60


def round_pairs(n, r):
    """(p, q) of round r in pair order, p < q; the bye is the pair with q == n"""
    m = n + (n & 1)
    pairs = [(m - 1, r)] + [((r + i) % (m - 1), (r - i + m - 1) % (m - 1)) for i in range(1, m // 2)]
    return np.array([(min(x, y), max(x, y)) for x, y in pairs], dtype=np.int64)


def sort_signs(d, v):
    """the tail both solvers share: stable by descending eigenvalue, each column's largest entry (the first) positive"""
    order = np.argsort(-d, kind="stable")
    v = v[:, order]
    big = np.argmax(np.abs(v), axis=0)
    neg = v[big, np.arange(v.shape[1])] < 0.0
    return d[order], np.where(neg[None, :], -v, v)


def sym_eig_par(a):
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    v = np.eye(n)
    scale = np.float64(0.0)
    for i in range(n):
        scale = scale + abs(a[i, i])
    thr = scale * 2.0 ** -70
    m = n + (n & 1)
    sweeps = 0
    while sweeps < EIG_SWEEPS:
        sweeps += 1
        rotated = False
        for r in range(m - 1):
            pq = round_pairs(n, r)
            order = np.empty(m, dtype=np.int64)             # the place of an index's pair in the round
            order[pq[:, 0]] = order[pq[:, 1]] = np.arange(len(pq))
            pq = pq[pq[:, 1] < n]
            pq = pq[np.abs(a[pq[:, 0], pq[:, 1]]) > thr]
            if not len(pq):
                continue
            rotated = True
            p, q = pq[:, 0], pq[:, 1]
            app, aqq, apq = a[p, p], a[q, q], a[p, q]
            theta = (aqq - app) / (2.0 * apq)
            t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            rp, rq = a[p, :], a[q, :]                       # the row side
            a[p, :], a[q, :] = c[:, None] * rp - s[:, None] * rq, s[:, None] * rp + c[:, None] * rq
            cp, cq = a[:, p], a[:, q]                       # the column side
            a[:, p], a[:, q] = c[None, :] * cp - s[None, :] * cq, s[None, :] * cp + c[None, :] * cq
            later = order[:n, None] > order[None, :n]       # the blocks of a later pair before an earlier one: the mirror
            a = np.where(later, a.T, a)
            tap = t * apq                                   # a rotated pair's own block
            a[p, p], a[q, q] = app - tap, aqq + tap
            a[p, q] = a[q, p] = 0.0
            vp, vq = v[:, p], v[:, q]
            v[:, p], v[:, q] = c[None, :] * vp - s[None, :] * vq, s[None, :] * vp + c[None, :] * vq
        if not rotated:
            break
    lam, v = sort_signs(np.diag(a).copy(), v)
    return lam, v, sweeps
