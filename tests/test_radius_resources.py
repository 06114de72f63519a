"""Compiler resource remarks of the radius-search kernels (no GPU needed: hipcc cross-compiles for gfx950): exactly these
twenty kernels, no scratch, no spills, and the registers, static LDS and waves per SIMD that DESIGN.md 3.1 states.  The
kernels that size their LDS at launch (traverse_kernel, fused_kernel) report 0 bytes here."""
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# name -> (VGPRs, static LDS bytes per workgroup, the compiler's waves per SIMD)
KERNELS = {"bbox_partial_kernel<true>": (31, 96, 8),
           "bbox_partial_kernel<false>": (31, 96, 8),
           "grid_setup_kernel": (42, 2056, 8),
           "bin_init2_kernel": (8, 0, 8),
           "coarse_kernel<false>": (31, 16400, 8),
           "coarse_kernel<true>": (48, 16400, 8),
           "sup_scan_kernel": (41, 68, 8),
           "fine_kernel": (108, 34832, 4),
           "traverse_kernel<128, false, true>": (45, 0, 8),
           "traverse_kernel<128, true, true>": (59, 0, 8),
           "traverse_kernel<128, true, false>": (59, 0, 8),
           "fused_kernel<64>": (120, 0, 4),
           "tq_kernel<32, true, false>": (96, 10496, 4),
           "tq_kernel<32, false, false>": (126, 10496, 4),
           "tq_kernel<64, true, false>": (158, 13704, 3),
           "tq_kernel<64, false, false>": (156, 13704, 3),
           "tq_kernel<64, true, true>": (161, 13704, 3),
           "tq_expand_kernel": (22, 512, 8),
           "reduce_stats_kernel": (34, 192, 8),
           "pad_fill_kernel": (4, 0, 8)}


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "radius_neighbors.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(.+?)\s+((?:[A-Za-z][A-Za-z ]*=\d+\s*)+)$", line)  # (template arguments hold blanks)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z][A-Za-z ]*)=(\d+)", m.group(2))}
    return rows


def test_radius_kernels():
    rows = _resources()
    assert sorted(rows) == sorted(KERNELS), sorted(rows)
    for name, v in rows.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert (v["VGPRs"], v["LDS Size"], v["Occupancy"]) == KERNELS[name], (name, v)


def test_documented_figures_match():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 3.1 radius_neighbors"):text.index("### 3.2 grid_subsampling")]
    for name, (vgprs, lds, waves) in KERNELS.items():
        row = next(line for line in section.splitlines() if line.startswith(f"| `{name}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert cells[1:4] == [str(vgprs), f"{lds} B", str(waves)], row
