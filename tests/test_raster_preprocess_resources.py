"""Compiler resource remarks of the rasterizer's preprocess (no GPU needed: hipcc cross-compiles for gfx950).  The
multi-view instances hold 48 SH coefficients per thread across the view loop; they must stay at >= 4 waves per SIMD with
no scratch, and the LDS of a block must still let four blocks share a CU."""
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _preprocess_resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "rasterizer.hip",
                        "preprocess_kernel"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(preprocess_kernel<[^>]*>)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_multi_view_preprocess_occupancy_and_no_spills():
    rows = _preprocess_resources()
    multi = {k: v for k, v in rows.items() if k.endswith("false>")}   # LATE = false
    assert len(multi) == 6, sorted(rows)
    for name, v in multi.items():
        assert v["Occupancy"] >= 4, (name, v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
        assert 4 * v["LDS Size"] <= 160 * 1024, (name, v)
    for name, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
