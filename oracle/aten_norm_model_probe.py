#!/usr/bin/env python3
"""What torch.norm does on a contiguous fp32 CPU tensor, and how well the product's models of it hold.

TEST INFRASTRUCTURE (like everything under oracle/): run by hand, its output is quoted in DESIGN.md 6.3 and in
shardmerge_amd/csrc/sm_aten_norm.hpp / sm_select.hpp.  Three parts:

(a) the STRUCTURE of ATen's kernel, established on random vectors: acc = fma(x, x, acc) in 8 serial fp32 lanes, lanes
    added in order, then the T = n % 8 tail elements - the first 4 * (T // 4) as a rounded product and an add, the
    rest as fma - and the square root.  (What the exact parallel emulation, k_aten_*, reproduces bit for bit.)
(b) the norms of the GATHERED slerp-class vectors (reference functions.py:36,40): torch.norm on the reference's own
    gathered vectors against (i) the ordered emulation over the half-spectrum planes and (ii) the empirical
    mean-field model from sampled statistics (k_class_emf + emf_norm_ratio).
(c) the Gaussian mean-field model of a K >= 3 intermediate's norm (aten_gauss_norm_ratio) against torch.norm on
    Gaussian data and on a real intermediate of the oracle.

usage: python oracle/aten_norm_model_probe.py [size]      (size: the square test shape, default 2048)
"""
import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import torch
from scipy.special import erfc

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from oracle import spectral_oracle as so  # noqa: E402

f32 = np.float32


def _rnd(v: Fraction):
    f = f32(float(v))
    cands = [np.nextafter(f, f32(-np.inf)), f, np.nextafter(f, f32(np.inf))]
    return f32(min(cands, key=lambda c: (abs(Fraction(float(c)) - v), int(f32(c).view(np.uint32)) & 1)))


def _fma(a, b, c):
    return _rnd(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def aten_structure(x: np.ndarray):
    n = len(x)
    nv = n - n % 8
    acc = [f32(0)] * 8
    for row in x[:nv].reshape(-1, 8):
        acc = [_fma(row[j], row[j], acc[j]) for j in range(8)]
    t = acc[0]
    for j in range(1, 8):
        t = f32(t + acc[j])
    tail = x[nv:]
    g = (len(tail) // 4) * 4
    for v in tail[:g]:
        t = f32(t + f32(v * v))
    for v in tail[g:]:
        t = _fma(v, v, t)
    return float(np.sqrt(t))


def part_a():
    torch.manual_seed(11)
    ok = tot = 0
    for n in [8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 23, 31, 100, 1003, 4099]:
        for _ in range(20):
            x = torch.randn(n) * 0.003
            tot += 1
            ok += aten_structure(x.numpy()) == torch.norm(x).item()
    print(f"(a) fma lanes + in-order lanes + tail (4-blocks rounded product, rest fma): {ok}/{tot} random vectors bit-equal to torch.norm")


def gauss_G(rho):
    if rho < 1e-6:
        return 1.0
    k = np.arange(int(80.0 / rho) + 4, dtype=np.float64)
    return rho * erfc(np.sqrt((k + 0.5) * rho / 2.0)).sum()


def gauss_ratio(n, sigma):
    m, s2 = n // 8, sigma * sigma
    S, left, e = 0.0, float(m), math.floor(math.log2(s2)) - 2
    while left > 0:
        hi = 2.0 ** (e + 1)
        if S >= hi:
            e += 1
            continue
        g = s2 * gauss_G(2.0 ** (e - 23) / s2)
        need = (hi - S) / g
        if need >= left:
            S, left = S + left * g, 0
        else:
            S, left, e = hi, left - need, e + 1
    return math.sqrt(S / (s2 * m))


def emf_ratio(y, w, nfull, sample_keep=None):
    """empirical mean-field: y = squares of the class values (plane order), w = their multiplicities (0 outside)"""
    if sample_keep is not None:
        ys, ws = y[sample_keep], w[sample_keep]
    else:
        ys, ws = y, w
    cnt_s, s_s, cnt = ws.sum().item(), (ys * ws).sum().item(), w.sum().item()
    N, mean_y = math.floor(cnt / 8.0), s_s / cnt_s
    elo = math.floor(math.log2(0.03 * nfull + 1.0)) - 11
    g = {}
    for k in range(16):
        u = 2.0 ** (elo + k - 23)
        g[elo + k] = (torch.floor(ys / u + 0.5) * ws).sum().item() * u / cnt_s
    S, left, e = 0.0, float(N), math.floor(math.log2(mean_y)) - 2
    while left > 0:
        hi = 2.0 ** (e + 1)
        if S >= hi:
            e += 1
            continue
        ge = g.get(e, mean_y)
        need = (hi - S) / ge
        if need >= left:
            S, left = S + left * ge, 0
        else:
            S, left, e = hi, left - need, e + 1
    return math.sqrt(S / (N * mean_y))


def part_b(size):
    R = C = size
    base, fts = so.synthetic_layer(R, C, 2, seed=4000 + R)
    d = [(f.float() - base.float()) for f in fts]
    na, nb = d[0].norm().item(), d[1].norm().item()
    if na < nb:
        d, na, nb = d[::-1], nb, na
    f0, f1 = so.fft_transform(d[0] / na), so.fft_transform(d[1] / nb)
    r0, r1 = f0.real, f1.real
    thr = so.kth_smallest(torch.cat([r0.abs(), r1.abs()]), 0.08)
    sel = (r0.sign() == r1.sign()) & ~(r1.abs() < thr)
    Cb = C // 2 + 1
    w = torch.full((Cb, 1), 2.0, dtype=torch.float64)
    w[0] = w[C // 2] = 1.0
    m = sel[:, :Cb].t().double() * w
    rows = torch.arange(Cb * R // 8)
    print(f"(b) slerp class of a {R}x{C} K=2 pair: {int(sel.sum())} of {R * C} bins")
    for name, r in (("v0", r0), ("v1", r1)):
        g = r[sel]
        t, ex = g.norm().item(), g.double().norm().item()
        h = torch.where(sel, r, torch.zeros_like(r))[:, :Cb].t().contiguous()          # our plane order [Cb][R]
        # (i) ordered emulation: twins twice in a row (same lane), bins outside the class add an exact zero
        a2 = torch.stack([h[1:C // 2].reshape(-1, 8)] * 2, 1).reshape(-1)
        ordered = torch.cat([h[0].reshape(-1), a2, h[C // 2].reshape(-1)]).norm().item()
        y = (h.double() * h.double()).reshape(-1)
        full = math.sqrt((y * m.reshape(-1)).sum().item()) * emf_ratio(y, m.reshape(-1), R * C)
        keep = ((rows // 8) % 16 == 0).repeat_interleave(8)
        samp = math.sqrt((y * m.reshape(-1)).sum().item()) * emf_ratio(y, m.reshape(-1), R * C, keep)
        print(f"    {name}: torch.norm bias {(t - ex) / ex:+.3e} | ordered emulation err {(ordered - t) / t:+.2e} | "
              f"mean-field (all bins) {(full - t) / t:+.2e} | mean-field (1 piece in 16) {(samp - t) / t:+.2e}")


def part_c(size):
    torch.manual_seed(1)
    print("(c) Gaussian mean-field model of torch.norm's bias")
    for n in (1 << 22, 1 << 24, 1 << 26):
        for sigma in (0.002, 0.003):
            g = torch.randn(n) * sigma
            ex = g.double().norm().item()
            print(f"    n = {n:>9}, sigma = {sigma}: torch {(g.norm().item() - ex) / ex:+.4e}   model {gauss_ratio(n, sigma) - 1:+.4e}")
    base, fts = so.synthetic_layer(size, size, 2, seed=77)
    d = [(f.float() - base.float()) for f in fts]
    na, nb = d[0].norm().item(), d[1].norm().item()
    if na < nb:
        d = d[::-1]
    with so.fast_select():
        mrg, _, _ = so.merge_tensors_fft2_slerp(d[0], d[1], t=0.375, cutoff_pct=0.08, cull_pct=0.2)
    mrg = mrg * ((na + nb) / 2)
    ex = mrg.double().norm().item()
    print(f"    a real K = 3 intermediate ({size}x{size}): torch {(mrg.norm().item() - ex) / ex:+.4e}   "
          f"model {gauss_ratio(mrg.numel(), ex / math.sqrt(mrg.numel())) - 1:+.4e}")


if __name__ == "__main__":
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    part_a()
    part_b(size)
    part_c(size)
