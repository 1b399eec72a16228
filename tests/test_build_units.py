"""What each kernel translation unit of csrc is built from: a dependency-only pass of the compiler over every unit
(nothing is compiled).  The kernel units never parse the host orchestration, the static-plan units no operator, and
the operator groups none of the spectral pipeline's kernel headers - so that an edit recompiles what uses it."""
import os
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "shardmerge_amd" / "csrc"
MAKEFILE = (CSRC / "Makefile").read_text()
HIPCC = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", MAKEFILE, re.M).group(1)
NPLANS = int(re.search(r"^NPLANS = (\d+)", MAKEFILE, re.M).group(1))
NSIDE = int(re.search(r"^.define SM_SIDE_GROUPS (\d+)", (CSRC / "smhip_device.hpp").read_text(), re.M).group(1))

HOST_ONLY = {"sm_pipeline.hpp", "sm_delta_host.hpp", "sm_capi.inc", "shardmerge_hip.h"}
OPERATORS = {"sm_ties.hpp", "sm_dare.hpp", "sm_breadcrumbs.hpp", "sm_geo.hpp", "sm_sphere.hpp", "sm_sce.hpp", "sm_della.hpp",
             "sm_consensus.hpp", "sm_stats.hpp", "sm_extract.hpp", "sm_fusion.hpp", "sm_pcb.hpp", "sm_tsv.hpp", "sm_widen.hpp",
             "sm_cabs.hpp", "sm_iso.hpp", "sm_dpack.hpp", "sm_delta.hpp", "sm_lora.hpp", "sm_aten_norm.hpp"}
PIPELINE_KERNELS = {"sm_kernels.hpp", "sm_select.hpp", "sm_merge.hpp"}       # the kernel headers of the spectral pipeline
OPERATOR_GROUPS = range(7, 17)

UNITS = [(f"inst_{i}", f"-DSM_PLAN_INDEX={i}", "smhip_inst.hip") for i in range(NPLANS)] + \
        [(f"side_{g}", f"-DSM_SIDE_GROUP={g}", "smhip_side.hip") for g in range(NSIDE)]


def unit_files(define, source):
    """base names of the files the unit is built from (make-rule output of the host and the device pass)"""
    r = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-MM", define, source], cwd=CSRC,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = {Path(tok).name for tok in r.stdout.replace("\\\n", " ").split() if not tok.endswith(":")}
    assert source in files and "smhip_device.hpp" in files, r.stdout       # the rule was read, not an empty output
    return files


@pytest.mark.parametrize("name,define,source", UNITS, ids=[u[0] for u in UNITS])
def test_kernel_unit_includes_only_what_it_builds(name, define, source):
    files = unit_files(define, source)
    assert not files & HOST_ONLY, f"{name} parses host-only files: {sorted(files & HOST_ONLY)}"
    if name.startswith("inst_"):
        assert not files & OPERATORS, f"{name} parses operator headers: {sorted(files & OPERATORS)}"
    elif int(name[5:]) in OPERATOR_GROUPS:
        assert not files & PIPELINE_KERNELS, f"{name} parses the spectral pipeline's kernels: {sorted(files & PIPELINE_KERNELS)}"

