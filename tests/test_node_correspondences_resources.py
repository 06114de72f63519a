"""Compiler resource remarks of csrc/node_correspondences.hip (no GPU needed: hipcc cross-compiles for gfx950): no scratch,
no spilled registers, the 3 KB of LDS of one staged reference patch, and a register count that lets two 256-thread
workgroups of the pair kernel -- 4 waves each, one per SIMD -- share a compute unit with room to spare (8 waves per SIMD)."""
import os
import re
import subprocess
import sys

from gaussreg_amd import matching  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "node_correspondences.hip", "nc_"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\w+)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_node_correspondence_kernels_resources():
    rows = _resources()
    assert sorted(rows) == ["nc_compact_kernel", "nc_pair_kernel", "nc_prepare_kernel"], sorted(rows)
    for name, v in rows.items():
        print(f"{name}: VGPRs {v['VGPRs']}  SGPRs {v['TotalSGPRs']}  LDS {v['LDS Size']}  scratch {v['ScratchSize']}  "
              f"waves/SIMD {v['Occupancy']}")
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    p = rows["nc_pair_kernel"]
    # 256 threads = 4 waves, one per SIMD: at 64 registers or fewer eight such workgroups fit a compute unit
    assert p["VGPRs"] + p["AGPRs"] <= 64 and p["Occupancy"] == 8, p
    assert p["LDS Size"] <= 3 * 256 * 4 + 64, p       # x, y, z of at most 256 reference points and the wave counters
    assert rows["nc_prepare_kernel"]["LDS Size"] == 0 and rows["nc_compact_kernel"]["LDS Size"] == 0
