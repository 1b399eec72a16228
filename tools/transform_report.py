#!/usr/bin/env python3
"""The per-bin transform conformance as a table: the cases of tests/transform_checks.py, and per case and family the
worst e(kernel), E_ref (torch's fp32 FFT / the fp32 oracle on the same inputs) and their ratio; the tests assert
ratio <= 4 (one stated exception: transform_checks.direct_sum_margin).

    python tools/transform_report.py --device cuda > profiles/transform_conformance.txt
    python tools/transform_report.py --device cpu  > profiles/transform_conformance_emulator.txt

--device cpu runs the work-group emulator with the batching and the input lists of tests/test_transform_host.py."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tests import transform_checks as tc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", default="cuda", help="cuda: the HIP library; cpu: the work-group emulator")
    ns = ap.parse_args()
    if ns.device == "cpu":
        from tests.emul.loader import emul_engine
        eng, tier, _batched = emul_engine(), "emulator", tc.emulator_batched
    else:
        from shardmerge_amd.engine import get_engine
        eng, tier, _batched = get_engine("cuda:0"), "device", lambda shape, axis: False
    worst = {}

    def show(case, records, prefix=""):
        for fam, (ek, er) in tc.pooled(records).items():
            fam = prefix + fam
            ratio = ek / er if er > 0 else (0.0 if ek == 0 else float("inf"))
            print(f"{case:34s} {fam:12s} e(kernel) {ek:.3e}  E_ref {er:.3e}  ratio {ratio:5.2f}")
            if ratio > worst.get(fam, (0.0, ""))[0]:
                worst[fam] = (ratio, case)

    print(f"# tier: {tier}; margin {tc.MARGIN}; torch {torch.__version__}")
    print("# plain transforms: fft_transform / ifft_transform against the fp64 DFT, E_ref from torch's fp32 FFT")
    for shape, axis in tc.fn_shapes():
        b = _batched(shape, axis)
        show(f"{tc.shape_id(shape)} axis {axis}{' batched' if b else ''}", tc.engine_records(eng, shape, axis, batched=b))
    for n in tc.MISALIGNED_LENGTHS:
        for shape, axis in (((2, n), 1), ((n, 2), 0)):
            b = _batched(shape, axis)
            show(f"misaligned {tc.shape_id(shape)}{' batched' if b else ''}",
                 tc.engine_records(eng, shape, axis, place=tc.misaligned_on(eng), batched=b))
    print("# merge-only paths: the arithmetic-branch closed form in fp64, E_ref from the fp32 oracle")
    for shape in tc.FOLDED_SHAPES:
        rec, _, _ = tc.merge_records(eng, shape, {"folded": tc.FOLD_ON, "plain": tc.FOLD_OFF})
        for v in rec:
            show(f"{tc.shape_id(shape)} {v}", rec[v], "merge_")
    if tier == "device":
        for shape in tc.UNHOOKED_DEVICE_SHAPES:
            rec, _, _ = tc.merge_records(eng, shape, {"default": {}})
            show(f"{tc.shape_id(shape)} no hook", rec["default"], "merge_")
    for cid, shape, variants, _, _ in tc.PATH_CASES:
        rec, _, _ = tc.merge_records(eng, shape, variants)
        for v in rec:
            show(f"{cid} {v}", rec[v], "merge_")
    print("# worst ratio per family")
    for fam, (ratio, case) in sorted(worst.items()):
        print(f"{fam:12s} {ratio:5.2f}  at {case}")


if __name__ == "__main__":
    main()
