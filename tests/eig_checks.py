"""The checks of the device-side eigensolver (Engine.sym_eig, smhip_sym_eig_par; csrc/sm_eig.hpp), shared by the emulator
and the MI355X tests: bit for bit against tests/eig_oracle.py, the accuracy against numpy.linalg.eigh held to 4 x the
cyclic host solver's on the same matrices, and the operators that use it (tsv, extract-lora)."""
import functools

import numpy as np
import pytest
import torch

from tests import eig_oracle as eo

# odd n: the bye; 96 | 97 and 128 | 129: both sides of a residency plan's boundary; 272: the largest
SIZES = (1, 2, 3, 5, 16, 79, 80, 96, 97, 128, 129, 272)
KINDS = ("flat", "graded", "rank_half", "diagonal", "rank_one", "neg_zero")
CASES = [(n, kind) for n in SIZES for kind in KINDS]
ACCURACY_SIZES = (80, 129, 272)


@functools.lru_cache(maxsize=None)
def matrix(n, kind, seed=0):
    """Grams P^T P of Gaussian fp32 panels, taken in fp64 (both triangles equal bit for bit)"""
    rng = np.random.default_rng([n, KINDS.index(kind), seed])
    panel = lambda cols: rng.standard_normal((4 * n + 8, cols)).astype(np.float32)
    if kind == "diagonal":                                  # one sweep, nothing rotates; a tie and a negative value
        d = np.round(rng.standard_normal(n) * 4.0)
        return np.diag(d)
    if kind == "rank_one":                                  # identity plus a rank-one term: n - 1 equal eigenvalues
        u = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        a = np.eye(n) + np.outer(u, u)
    else:
        p = panel(n)
        if kind == "graded":                                # 12 decades, what orth sees after a power step
            p = p * (10.0 ** (-6.0 * np.arange(n) / max(n - 1, 1))).astype(np.float32)
        if kind == "rank_half":                             # half the eigenvalues at rounding level
            h = (n + 1) // 2
            p = (panel(h) @ rng.standard_normal((h, n)).astype(np.float32)).astype(np.float32)
        p = p.astype(np.float64)
        a = p.T @ p
    a = np.triu(a) + np.triu(a, 1).T
    if kind == "neg_zero":                                  # a Gram block beside a diagonal one, joined by zeros of both signs
        h = n // 2
        a[:h, h:] = 0.0
        a[h:, :h] = 0.0
        i, j = np.indices((n, n))
        a[(i != j) & ((i < h) != (j < h)) & ((i + j) % 3 == 0)] = -0.0
        a[(i != j) & (i >= h) & (j >= h)] = np.where((i + j) % 2 == 0, -0.0, 0.0)[(i != j) & (i >= h) & (j >= h)]
    return a


@functools.lru_cache(maxsize=None)
def oracle(n, kind, seed=0):
    return eo.sym_eig_par(matrix(n, kind, seed))


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def check_bits(eng, n, kind):
    lam, v, sweeps = eng.sym_eig(torch.from_numpy(matrix(n, kind)))
    want = oracle(n, kind)
    assert sweeps == want[2]
    assert np.array_equal(bits(lam.numpy()), bits(want[0]))
    assert np.array_equal(bits(v.numpy()), bits(want[1]))
    if kind == "diagonal":
        assert sweeps == 1 and sorted(np.abs(v.numpy()).sum(0)) == [1.0] * n and (v.numpy() >= 0).all()


def check_batch(eng):
    """three matrices of n = 80 in one launch, a work-group each"""
    kinds = ("flat", "graded", "rank_one")
    lam, v, sweeps = eng.sym_eig(torch.from_numpy(np.stack([matrix(80, k) for k in kinds])))
    for b, k in enumerate(kinds):
        want = oracle(80, k)
        assert int(sweeps[b]) == want[2]
        assert np.array_equal(bits(lam[b].numpy()), bits(want[0])) and np.array_equal(bits(v[b].numpy()), bits(want[1]))


def quality(a, lam, v):
    """(eigenvalue error / ||A||_2, ||A V - V diag(lam)||_F / ||A||_F, ||V^T V - I||_F) against numpy.linalg.eigh"""
    ref = np.linalg.eigh(a)[0][::-1]
    return (np.abs(lam - ref).max() / np.abs(ref).max(), np.linalg.norm(a @ v - v * lam[None, :]) / np.linalg.norm(a),
            np.linalg.norm(v.T @ v - np.eye(len(lam))))


def check_accuracy(eng, n, kind):
    """the new solver within 4 x the cyclic host solver on the same matrix: both are Jacobi in the same arithmetic, so a
    factor covers the other ordering (the bound is the issue's; the measured values of both stand in the README)"""
    a = matrix(n, kind)
    lam_h, v_h, sw_h = eng.sym_eig(torch.from_numpy(a), method="host")
    lam_d, v_d, sw_d = eng.sym_eig(torch.from_numpy(a), method="device")
    host, dev = quality(a, lam_h.numpy(), v_h.numpy()), quality(a, lam_d.numpy(), v_d.numpy())
    print(f"eig accuracy n={n} {kind}: host sweeps {sw_h} " + " ".join(f"{x:.2e}" for x in host) +
          f" | device sweeps {sw_d} " + " ".join(f"{x:.2e}" for x in dev))
    assert sw_d < eo.EIG_SWEEPS and sw_h < eo.EIG_SWEEPS
    for name, h, d in zip(("eigenvalues", "residual", "orthogonality"), host, dev):
        assert d <= 4.0 * h, (name, d, h)


def check_arguments(eng):
    a = torch.from_numpy(matrix(5, "flat"))
    for bad in (a.float(), a[:, :4], torch.zeros(273, 273, dtype=torch.float64), torch.zeros(0, 4, 4, dtype=torch.float64)):
        with pytest.raises(ValueError):
            eng.sym_eig(bad)
    with pytest.raises(ValueError):
        eng.sym_eig(a, method="lapack")
    nan = a.clone()
    nan[1, 2] = nan[2, 1] = float("nan")
    for method in ("host", "device"):
        with pytest.raises(ValueError):
            eng.sym_eig(nan, method=method)
    dll = eng.lib.dll
    assert dll.smhip_sym_eig_par_workspace(0, 1) == 0 and dll.smhip_sym_eig_par_workspace(273, 1) == 0
    assert dll.smhip_sym_eig_par_workspace(80, 0) == 0 and dll.smhip_sym_eig_par_workspace(272, 3) >= 3 * 2 * 272 * 273 * 8
    assert eig_launches(eng, 3) == 1


def eig_launches(eng, batch):
    """the whole iteration of a batch is ONE launch"""
    from tests.harness import profile_of
    a = torch.from_numpy(np.stack([matrix(16, "flat")] * batch))
    return profile_of(eng, lambda: eng.sym_eig(a))["eig_jacobi"]


# ---- through the operators: the fixtures and the tolerances of tests/tsv_checks.py and of the extraction's tests ----
def tsv_inputs(rows, cols, k):
    """fp32 deltas of rank 12 plus noise over a zero base, as tsv_checks.property_inputs at another shape"""
    g = torch.Generator().manual_seed(4100 + k + rows)
    low = lambda: (torch.randn(rows, 12, generator=g) / torch.arange(1, 13) ** 0.5) @ torch.randn(12, cols, generator=g) / 12 ** 0.5
    return [0.02 * (low() + 0.05 * torch.randn(rows, cols, generator=g)) for _ in range(k)], [torch.zeros(rows, cols)] * k


def tsv_device(eng, fts, bases, alphas, r, eig="device"):
    from tests import tsv_checks as tc
    same = {}
    dev = lambda t: same.setdefault(id(t), tc.on(eng, t))
    out, rep, delta = eng.tsv_merge([dev(t) for t in fts], [dev(t) for t in bases], alphas, dev(bases[0]), rank=r, power_iters=2,
                                    key=tc.KEY, want_delta=True, eig=eig)
    return tc.host(out), tc.host(delta).double(), rep


def check_tsv_singular_values(eng, rows, cols, k=3, r=16):
    """the R leading singular values of the merged delta are the sorted alpha_i sigma_ij"""
    from tests import tsv_checks as tc
    fts, bases = tsv_inputs(rows, cols, k)
    alphas = list(tc.ALPHAS[:k])
    _, merged, rep = tsv_device(eng, fts, bases, alphas, r)
    s = [a * x for a, sig, rho in zip(alphas, rep.sigma, rep.rho) for x in sig[:rho]]
    dev, tail, fro = tc.singular_value_figures(merged, s)
    print(f"tsv_eig device {rows}x{cols} k={k}: R {rep.R}, deviation {dev:.2e}, next {tail:.2e}, Frobenius {fro:.2e}")
    assert rep.R == r * k == rep.kept_U == rep.kept_W
    assert dev <= tc.SV_TOL and tail <= tc.TAIL_TOL and fro <= tc.FRO_TOL, (dev, tail, fro)


def check_tsv_duplicates(eng):
    """two identical finetunes give the k = 1 result"""
    from tests import tsv_checks as tc
    fts, bases = tsv_inputs(128, 512, 1)
    _, both, rep = tsv_device(eng, [fts[0], fts[0]], [bases[0]] * 2, [1.0, 1.0], 16)
    _, one, rep1 = tsv_device(eng, fts, bases, [1.0], 16)
    assert rep.R == 32 and rep.kept_U == rep.kept_W == 16 == rep1.R
    assert float(torch.linalg.norm(both - one) / torch.linalg.norm(one)) <= tc.DUP_TOL


def check_tsv_host_is_unchanged(eng):
    """eig="host" is the call without the argument, byte for byte; "device" is another function"""
    from tests import tsv_checks as tc
    fts, bases = tsv_inputs(128, 512, 2)
    alphas = [0.5, 0.3]
    out_h, _, rep_h = tsv_device(eng, fts, bases, alphas, 16, eig="host")
    out_0, rep_0 = eng.tsv_merge([tc.on(eng, t) for t in fts], [tc.on(eng, t) for t in bases], alphas, tc.on(eng, bases[0]), rank=16,
                                 power_iters=2, key=tc.KEY)
    assert torch.equal(tc.raw(out_h), tc.raw(tc.host(out_0))) and rep_h == rep_0
    with pytest.raises(ValueError):
        tsv_device(eng, fts, bases, alphas, 16, eig="gpu")


def check_tsv_against(eng, other, rows=300, cols=4544, k=2, r=64):
    """the emulator library and the MI355X give the same bytes under eig = device"""
    from tests import tsv_checks as tc
    fts, bases = tc.merge_inputs(rows, cols, k, seed=1)
    got = [tsv_device(e, fts, [bases[0]] * k, list(tc.ALPHAS[:k]), r) for e in (eng, other)]
    assert torch.equal(tc.raw(got[0][0]), tc.raw(got[1][0])) and torch.equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]


def check_extract_exact_rank(eng):
    """extract-lora on the exact rank-16 input recovers rank 16 within the extraction's own residual bound (4e-6)"""
    from tests import extract_checks as xc
    ft, base, D, sv = xc.quality_inputs()["exact16"]
    a, b, rep = eng.lora_extract(xc.on(eng, ft), xc.on(eng, base), 24, power_iters=2, factor_dtype=torch.float32, name="exact16", eig="device")
    a, b = xc.host(a), xc.host(b)
    assert rep.effective_rank == 16 and not a[16:].any() and not b[:, 16:].any()
    assert float(torch.linalg.norm(D - b.double() @ a.double()) / torch.linalg.norm(D)) <= 4e-6


def check_config(tmp_path):
    """tsv_eig: host | device with operator tsv alone; the two settings never share a resumed run"""
    import click
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.distributed import config_stamp
    from tests.harness import yaml_config
    stamps = set()
    for opts in ({"operator": "tsv"}, {"operator": "tsv", "tsv_eig": "host"}, {"operator": "tsv", "tsv_eig": "device"}):
        cfg = MergeConfig.from_yaml(yaml_config(tmp_path, opts))
        assert cfg.merge_options == {k: v for k, v in opts.items() if k != "operator"}
        stamps.add(config_stamp(cfg))
    assert len(stamps) == 3
    for opts, text in (({"operator": "tsv", "tsv_eig": "lapack"}, "host | device"), ({"operator": "tsv", "tsv_eig": 1}, "host | device"),
                       ({"operator": "ties", "tsv_eig": "device"}, "accepted only with operator: tsv"),
                       ({"operator": "iso_c", "tsv_eig": "device"}, "accepted only with operator: tsv")):
        with pytest.raises(click.BadParameter, match=text):
            MergeConfig.from_yaml(yaml_config(tmp_path, opts))


def check_cli(tmp_path, eng, device=None):
    """`merge` with tsv_eig: host writes the bytes of a config without the key; with device it runs, and names the solver"""
    from tests import lora_fixtures as lf
    from tests import tsv_checks as tc
    from tests.harness import run_cli
    lf.setup_k3(tmp_path, eng)
    outs = {}
    for tag, extra in (("plain", {}), ("host", {"tsv_eig": "host"}), ("device", {"tsv_eig": "device"})):
        res = run_cli(tc.write_config(tmp_path, "org/lora_full", tag, {**tc.OPTIONS, **extra}, device))
        assert res.exit_code == 0, res.output
        outs[tag] = lf.read_outputs(tmp_path / tag)
    for name in outs["plain"]:
        assert torch.equal(tc.raw(outs["plain"][name]), tc.raw(outs["host"][name])), name
        assert outs["device"][name].shape == outs["plain"][name].shape
        close = (outs["device"][name].float() - outs["plain"][name].float()).abs().max() <= 2.0 ** -7 * outs["plain"][name].float().abs().max()
        assert close, name                                  # (bf16 outputs: the solvers differ by rounding, one ulp of the largest)
    assert "eigensolver device" in (tmp_path / "device" / "README.md").read_text()
