"""Compiler resource remarks of the GroupNorm training kernels (no GPU needed: hipcc cross-compiles for gfx950): the four
kernels of csrc/group_norm_backward.hip and the statistics copy of csrc/kpconv.hip use no scratch, spill nothing, and stay at
or under the register and LDS counts DESIGN.md 3.5.1 records -- all of them leave eight waves per SIMD, which streaming
kernels want."""
import os
import re
import subprocess
import sys

from gaussreg_amd import kpconv_blocks  # noqa: F401  (the module whose kernels these are)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# kernel -> (VGPRs, LDS bytes per workgroup) as recorded in DESIGN.md 3.5.1
RECORDED = {
    "group_norm_bwd_sums_kernel<true>": (56, 16896),
    "group_norm_bwd_sums_kernel<false>": (56, 16896),
    "group_norm_bwd_fold_kernel": (24, 4096),
    "group_norm_bwd_finish_kernel": (26, 0),
    "group_norm_bwd_apply_kernel<true>": (44, 1024),
    "group_norm_bwd_apply_kernel<false>": (48, 1024),
    "group_norm_stats_copy_kernel": (6, 0),
}


def _resources(source, pattern):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), source, pattern],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\S+)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def test_group_norm_training_kernels_use_no_scratch_and_stay_within_the_record():
    rows = _resources("group_norm_backward.hip", "group_norm_bwd")
    rows.update(_resources("kpconv.hip", "group_norm_stats_copy"))
    assert sorted(rows) == sorted(RECORDED), sorted(rows)
    for name, v in rows.items():
        print(f"{name}: VGPRs {v['VGPRs']}  AGPRs {v['AGPRs']}  SGPRs {v['TotalSGPRs']}  LDS {v['LDS Size']}  "
              f"scratch {v['ScratchSize']}  waves/SIMD {v['Occupancy']}")
        vgprs, lds = RECORDED[name]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["VGPRs"] + v["AGPRs"] <= vgprs and v["LDS Size"] <= lds, (name, v)
        assert v["Occupancy"] == 8, (name, v)
