"""Compiler resource remarks of the generalised-ICP and covariance kernels (no GPU needed: hipcc cross-compiles for gfx950): their
names, no scratch, no spills, and the LDS, register count and waves per SIMD that DESIGN.md 3.15 states."""
import os
import re
import subprocess
import sys

from gaussreg_amd import icp  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# LDS bytes per workgroup, VGPRs, and the compiler's waves per SIMD
GICP = (("icp_init_kernel", {"LDS Size": 0, "VGPRs": 2, "Occupancy": 8}),
        ("icp_key_kernel", {"LDS Size": 1536, "VGPRs": 12, "Occupancy": 8}),
        ("icp_gather_kernel", {"LDS Size": 0, "VGPRs": 6, "Occupancy": 8}),
        ("icp_match_kernel", {"LDS Size": 0, "VGPRs": 43, "Occupancy": 8}),
        ("icp_fallback_kernel", {"LDS Size": 0, "VGPRs": 29, "Occupancy": 8}),
        ("icp_scatter_kernel", {"LDS Size": 0, "VGPRs": 8, "Occupancy": 8}),
        ("gicp_cov_kernel", {"LDS Size": 0, "VGPRs": 2, "Occupancy": 8}),
        ("icp_sums_kernel<Generalized>", {"LDS Size": 928, "VGPRs": 124, "Occupancy": 4}),
        ("icp_fold_kernel<Generalized>", {"LDS Size": 1736, "VGPRs": 122, "Occupancy": 4}))
COVARIANCES = (("cov_normals_kernel", {"LDS Size": 0, "VGPRs": 20, "Occupancy": 8}),
               ("gs_cov_kernel", {"LDS Size": 0, "VGPRs": 36, "Occupancy": 8}))
FILES = (("cloud_icp_gicp.hip", GICP), ("cloud_covariances.hip", COVARIANCES))


def _resources(source):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), source], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\S+)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_cloud_gicp_kernels():
    for source, kernels in FILES:
        rows = _resources(source)
        assert sorted(rows) == sorted(name for name, _ in kernels), (source, sorted(rows))
        for name, v in rows.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        for name, want in kernels:
            for key, figure in want.items():
                assert rows[name][key] == figure, (name, key, rows[name])


def test_documented_figures_match():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 3.15 generalised ICP"):text.index("## 4. Measurement")]
    for _, kernels in FILES:
        for name, want in kernels:
            row = next(line for line in section.splitlines() if line.startswith(f"| `{name}`"))
            cells = [c.strip() for c in row.strip("|").split("|")]
            assert cells[1] == f"{want['LDS Size']} B", row
            assert cells[2].split()[0] == str(want["VGPRs"]) and cells[3] == "0", row
            assert cells[4].split()[0] == str(want["Occupancy"]), row
