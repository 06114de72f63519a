"""Compiler resource remarks of the image-loss kernels (no GPU needed: hipcc cross-compiles for gfx950): no scratch, and
the LDS per workgroup, register count and waves per SIMD that DESIGN.md 3.6 states."""
import os
import re
import subprocess
import sys

from gaussreg_amd import image_loss  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LDS_PER_CU = 160 * 1024
# LDS bytes per workgroup, VGPRs, and the compiler's waves per SIMD (= workgroups of 4 waves per CU)
FORWARD = {"LDS Size": 25392, "VGPRs": 80, "Occupancy": 6}
BACKWARD = {"LDS Size": 23088, "VGPRs": 52, "Occupancy": 7}


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "image_loss.hip", "image_loss"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\w+)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_image_loss_kernels():
    rows = _resources()
    assert sorted(rows) == ["image_loss_backward_kernel", "image_loss_forward_kernel", "image_loss_reduce_kernel"], sorted(rows)
    for name, v in rows.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    for name, want in (("image_loss_forward_kernel", FORWARD), ("image_loss_backward_kernel", BACKWARD)):
        v = rows[name]
        for key, figure in want.items():
            assert v[key] == figure, (name, key, v)
        assert want["Occupancy"] * v["LDS Size"] <= LDS_PER_CU, (name, v)


def test_documented_figures_match():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 3.6 photometric loss"):text.index("## 4. Measurement")]
    for name, want in (("image_loss_forward_kernel", FORWARD), ("image_loss_backward_kernel", BACKWARD)):
        row = next(line for line in section.splitlines() if line.startswith(f"| `{name}`"))
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert cells[1].startswith(f"{want['LDS Size']:,}".replace(",", " ") + " B"), row
        assert cells[2].split()[0] == str(want["VGPRs"]) and cells[3] == "0", row
        assert cells[4].split()[0] == str(want["Occupancy"]), row
