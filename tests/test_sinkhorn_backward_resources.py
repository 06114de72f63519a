"""Compiler resource remarks of csrc/sinkhorn.hip's backward kernel (no GPU needed: hipcc cross-compiles for gfx950): no
scratch, no spilled vector registers, and a register count that leaves the two waves per SIMD its 512-thread workgroup
needs.  The forward kernels of the same file are reported as well and must stay free of scratch."""
import os
import re
import subprocess
import sys

from gaussreg_amd import sinkhorn  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "sinkhorn.hip", "sinkhorn"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\w+)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_sinkhorn_kernels_use_no_scratch():
    rows = _resources()
    assert sorted(rows) == ["sinkhorn_backward_kernel", "sinkhorn_kernel", "sinkhorn_small_kernel"], sorted(rows)
    for name, v in rows.items():
        print(f"{name}: VGPRs {v['VGPRs']}  SGPRs {v['TotalSGPRs']}  scratch {v['ScratchSize']}  waves/SIMD {v['Occupancy']}")
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (name, v)
    b = rows["sinkhorn_backward_kernel"]
    # 512 threads = 8 waves on 4 SIMDs: two waves per SIMD share 512 registers
    assert b["VGPRs"] + b["AGPRs"] <= 256 and b["Occupancy"] >= 2, b
