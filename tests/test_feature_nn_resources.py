"""Compiler resource remarks of the feature-space nearest-neighbour kernels (no GPU needed: hipcc cross-compiles for gfx950):
their names, no scratch, no spills, and the LDS, register count and waves per SIMD that DESIGN.md 3.12 states."""
import os
import re
import subprocess
import sys

from gaussreg_amd import feature_nn  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# LDS bytes per workgroup, VGPRs, and the compiler's waves per SIMD.  feature_nn_kernel<ALIGNED, ROWS, COLS>
KERNELS = (("fn_sqnorm_kernel", {"LDS Size": 0, "VGPRs": 8, "Occupancy": 8}),
           ("fn_finish_kernel", {"LDS Size": 0, "VGPRs": 15, "Occupancy": 8}),
           ("feature_nn_kernel<true, true, true>", {"LDS Size": 39424, "VGPRs": 230, "Occupancy": 2}),
           ("feature_nn_kernel<false, true, true>", {"LDS Size": 39424, "VGPRs": 232, "Occupancy": 2}),
           ("feature_nn_kernel<true, true, false>", {"LDS Size": 37376, "VGPRs": 188, "Occupancy": 2}),
           ("feature_nn_kernel<false, true, false>", {"LDS Size": 37376, "VGPRs": 190, "Occupancy": 2}),
           ("feature_nn_kernel<true, false, true>", {"LDS Size": 37376, "VGPRs": 157, "Occupancy": 3}),
           ("feature_nn_kernel<false, false, true>", {"LDS Size": 37376, "VGPRs": 159, "Occupancy": 3}))


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "feature_nn.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\S.*?)\s{2,}(TotalSGPRs=.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_feature_nn_kernels():
    rows = _resources()
    assert sorted(rows) == sorted(name for name, _ in KERNELS), sorted(rows)
    for name, v in rows.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["AGPRs"] == 0, (name, v)
    for name, want in KERNELS:
        for key, figure in want.items():
            assert rows[name][key] == figure, (name, key, rows[name])


def test_documented_figures_match():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 3.12 nearest neighbours in feature space"):text.index("## 4. Measurement")]
    for name, want in KERNELS:
        row = next(line for line in section.splitlines() if line.startswith(f"| `{name}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert cells[1] == f"{want['LDS Size']} B", row
        assert cells[2].split()[0] == str(want["VGPRs"]) and cells[3] == "0", row
        assert cells[4].split()[0] == str(want["Occupancy"]), row
