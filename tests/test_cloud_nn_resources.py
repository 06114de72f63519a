"""Compiler resource remarks of the cross-cloud search kernels (no GPU needed: hipcc cross-compiles for gfx950): their
names, no scratch, no spills, and the LDS, register count and waves per SIMD that DESIGN.md 3.10 states."""
import os
import re
import subprocess
import sys

from gaussreg_amd import cloud_nn  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# LDS bytes per workgroup, VGPRs, and the compiler's waves per SIMD
KERNELS = (("cloud_boundaries_kernel", {"LDS Size": 16384, "VGPRs": 22, "Occupancy": 8}),
           ("cloud_box_kernel", {"LDS Size": 0, "VGPRs": 21, "Occupancy": 8}),
           ("cloud_cell_kernel", {"LDS Size": 1536, "VGPRs": 10, "Occupancy": 8}),
           ("cloud_scatter_kernel", {"LDS Size": 0, "VGPRs": 12, "Occupancy": 8}),
           ("cloud_knn_query_kernel<1>", {"LDS Size": 0, "VGPRs": 44, "Occupancy": 8}),
           ("cloud_knn_query_kernel<3>", {"LDS Size": 0, "VGPRs": 50, "Occupancy": 8}),
           ("cloud_knn_query_kernel<5>", {"LDS Size": 0, "VGPRs": 61, "Occupancy": 8}),
           ("cloud_knn_query_kernel<8>", {"LDS Size": 0, "VGPRs": 70, "Occupancy": 7}),
           ("cloud_knn_fallback_kernel<1>", {"LDS Size": 0, "VGPRs": 29, "Occupancy": 8}),
           ("cloud_knn_fallback_kernel<3>", {"LDS Size": 0, "VGPRs": 35, "Occupancy": 8}),
           ("cloud_knn_fallback_kernel<5>", {"LDS Size": 0, "VGPRs": 39, "Occupancy": 8}),
           ("cloud_knn_fallback_kernel<8>", {"LDS Size": 0, "VGPRs": 48, "Occupancy": 8}),
           ("cloud_radius_kernel<false>", {"LDS Size": 0, "VGPRs": 41, "Occupancy": 8}),
           ("cloud_radius_kernel<true>", {"LDS Size": 0, "VGPRs": 21, "Occupancy": 8}),
           ("cloud_radius_order_kernel", {"LDS Size": 0, "VGPRs": 24, "Occupancy": 8}))


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "cloud_nn.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\S+)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_cloud_nn_kernels():
    rows = _resources()
    assert sorted(rows) == sorted(name for name, _ in KERNELS), sorted(rows)
    for name, v in rows.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    for name, want in KERNELS:
        for key, figure in want.items():
            assert rows[name][key] == figure, (name, key, rows[name])


def test_documented_figures_match():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 3.10 cross-cloud nearest neighbours"):text.index("## 4. Measurement")]
    for name, want in KERNELS:
        row = next(line for line in section.splitlines() if line.startswith(f"| `{name}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert cells[1] == f"{want['LDS Size']} B", row
        assert cells[2].split()[0] == str(want["VGPRs"]) and cells[3] == "0", row
        assert cells[4].split()[0] == str(want["Occupancy"]), row
