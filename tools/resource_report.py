#!/usr/bin/env python3
"""Registers / spills / scratch / occupancy / LDS of the transform kernels of one static plan, or of one group of the other kernels.
usage: tools/resource_report.py <plan index in SM_STATIC_PLANS> [extra hipcc flags]
       tools/resource_report.py side<group> [extra hipcc flags]      (SM_SIDE_KERNELS_<group>; the groups: the end of csrc/smhip_device.hpp)"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

csrc = Path(__file__).resolve().parents[1] / "shardmerge_amd" / "csrc"
idx = sys.argv[1] if len(sys.argv) > 1 else "6"
# the Makefile's own rule and flags for the unit (so -fno-slp-vectorize for the plans that are built with it, and only
# for those), into a temporary folder
with tempfile.TemporaryDirectory(prefix="resource_report_") as build:
    obj = f"{build}/side_{idx[4:]}.o" if idx.startswith("side") else f"{build}/inst_{idx}.o"
    extra = " ".join(["-Rpass-analysis=kernel-resource-usage", *sys.argv[2:]])
    r = subprocess.run(["make", f"BUILD={build}", f"EXTRA={extra}", obj], cwd=csrc, capture_output=True, text=True)
if r.returncode != 0:
    sys.exit(r.stdout + r.stderr)
txt = r.stderr


def field(blk, key):
    m = re.search(re.escape(key) + r":\s*(\d+)", blk)
    return m.group(1) if m else "?"


for blk in txt.split("Function Name:")[1:]:
    m = re.search(r"sm_kernelINS_(\w+?)INS_5SPlanILi(\d+)ELi(\d+)", blk)
    side = re.search(r"sm_kernelINS_\d+(\w+?)EEvN", blk)
    name = f"{m.group(1)}<{m.group(2)},{m.group(3)}>" if m else (side.group(1) if side else blk[:40])
    print(f"{name:22s} VGPRs {field(blk, 'VGPRs'):>4s}  AGPRs {field(blk, 'AGPRs'):>3s}  SGPRs {field(blk, 'SGPRs'):>3s}  spill {field(blk, 'VGPRs Spill'):>3s}  scratch {field(blk, 'ScratchSize [bytes/lane]'):>4s}"
          f"  waves/SIMD {field(blk, 'Occupancy [waves/SIMD]'):>2s}  LDS {field(blk, 'LDS Size [bytes/block]')}")
