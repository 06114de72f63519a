"""Compiler resource remarks of the structure embedding's backward kernels (no GPU needed: hipcc cross-compiles for gfx950):
no scratch, no spill of either register kind, and the LDS per workgroup, register count and waves per SIMD that DESIGN.md
3.5.2 states."""
import os
import re
import subprocess
import sys

from gaussreg_amd import embedding  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LDS_PER_CU = 160 * 1024
# LDS bytes per workgroup, VGPRs, and the compiler's waves per SIMD (= workgroups of 4 waves per CU)
FIGURES = {"geo_embedding_backward_kernel<0>": {"LDS Size": 29952, "VGPRs": 98, "Occupancy": 4},
           "geo_embedding_backward_kernel<1>": {"LDS Size": 29952, "VGPRs": 134, "Occupancy": 3},
           "geo_embedding_backward_kernel<2>": {"LDS Size": 29952, "VGPRs": 151, "Occupancy": 3},
           "geo_embedding_backward_reduce_kernel": {"LDS Size": 0, "VGPRs": 7, "Occupancy": 8}}


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "geo_embedding_backward.hip",
                        "geo_embedding_backward"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\S+)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_geo_embedding_backward_kernels():
    rows = _resources()
    assert sorted(rows) == sorted(FIGURES), sorted(rows)
    for name, v in rows.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["AGPRs"] == 0, (name, v)                     # the VGPR figure is the whole register count of a lane
        for key, figure in FIGURES[name].items():
            assert v[key] == figure, (name, key, v)
        assert FIGURES[name]["Occupancy"] * v["LDS Size"] <= LDS_PER_CU, (name, v)
    # three workgroups per CU resident, as the slab count assumes (gr_geo_embedding_backward_plan: 768 workgroups)
    assert min(FIGURES[f"geo_embedding_backward_kernel<{m}>"]["Occupancy"] for m in (0, 1, 2)) >= 3


def test_documented_figures_match():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 3.5.2 Transformer backward"):text.index("### 3.6 photometric loss")]
    for name, want in FIGURES.items():
        row = next(line.strip() for line in section.splitlines() if line.strip().startswith(f"| `{name}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert cells[1].startswith(f"{want['LDS Size']:,}".replace(",", " ") + " B"), row
        assert cells[2].split()[0] == str(want["VGPRs"]) and cells[3] == "0", row
        assert cells[4].split()[0] == str(want["Occupancy"]), row
