"""Compiler figures of tile_scatter_kernel (no GPU needed: hipcc cross-compiles for gfx950).

The 256-thread instances (many views per call) count their tiles with a per-wave difference grid instead of a walk of every
rectangle; six of their workgroups share a CU, so they must stay at <= 80 VGPRs without scratch, and they must be shorter
than the instances with the counting walk were.  The 1 024-thread instances (a few views per call) keep their per-lane
count loop and with it their registers and their instruction count.

Instructions of the device assembly (hipcc -O3 -ffp-contract=off -fPIC --cuda-device-only -S; every line of the kernel that
is neither a label, a directive nor a comment), <LANE_ORDERED, threads, SEG>, before the grid -> with it:

    <true, 256, 0 / 1 / 2>    10 846 / 11 268 / 11 058  ->  4 454 / 4 877 / 4 666
    <false, 256, 0 / 1 / 2>   11 832 / 12 255 / 12 041  ->  5 441 / 5 861 / 5 650   (296 -> 32 ds_add_u32 each)
    <true, 1024, 0 / 1 / 2>    3 165 /  3 717 /  3 411     unchanged, line for line; 60 VGPRs
    <false, 1024, 0 / 1 / 2>   4 153 /  4 706 /  4 396     unchanged, line for line; 48 / 56 / 56 VGPRs

The static count of the 256-thread instances is held below what it was with the walk; the figures of the 1 024-thread
instances are those of the compiler this was recorded with and are compared exactly."""
import functools
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WALK_256 = {("true", 0): 10846, ("true", 1): 11268, ("true", 2): 11058, ("false", 0): 11832, ("false", 1): 12255,
            ("false", 2): 12041}
WIDE_1024 = {("true", 0): (3165, 60), ("true", 1): (3717, 60), ("true", 2): (3411, 60), ("false", 0): (4153, 48),
             ("false", 1): (4706, 56), ("false", 2): (4396, 56)}


@functools.lru_cache(maxsize=None)
def _resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "rasterizer.hip",
                        "tile_scatter_kernel"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*tile_scatter_kernel<(true|false), (\d+), (\d)>\s+(.*)", line)
        if m:
            rows[(m.group(1), int(m.group(2)), int(m.group(3)))] = {k.strip(): int(v)
                                                                    for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(4))}
    assert len(rows) == 12, sorted(rows)
    return rows


@functools.lru_cache(maxsize=None)
def _instructions():
    """{(LANE_ORDERED, threads, SEG): instruction lines} from the device assembly."""
    src = os.path.join(ROOT, "gaussreg_amd", "csrc", "rasterizer.hip")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    counts, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"_ZN\w*19tile_scatter_kernelILb([01])ELi(\d+)ELi(\d)E\w*:", line)
        if m:
            cur = ("true" if m.group(1) == "1" else "false", int(m.group(2)), int(m.group(3)))
            counts[cur] = 0
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            code = line.split(";")[0].strip()
            if code and not code.startswith(".") and not code.endswith(":"):
                counts[cur] += 1
    assert len(counts) == 12, sorted(counts)
    return counts


def test_many_view_scatter_fits_six_workgroups_and_lost_the_counting_walk():
    rows, counts = _resources(), _instructions()
    for (lo, seg), before in WALK_256.items():
        v = rows[(lo, 256, seg)]
        assert v["VGPRs"] <= 80 and v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0 and v["Occupancy"] >= 6, (lo, seg, v)
        assert counts[(lo, 256, seg)] < before, (lo, seg, counts[(lo, 256, seg)], before)


def test_few_view_scatter_is_the_one_it_was():
    rows, counts = _resources(), _instructions()
    for (lo, seg), (n, vgprs) in WIDE_1024.items():
        v = rows[(lo, 1024, seg)]
        assert v["VGPRs"] == vgprs and v["VGPRs Spill"] == 0 and v["ScratchSize"] == 0, (lo, seg, v)
        assert counts[(lo, 1024, seg)] == n, (lo, seg, counts[(lo, 1024, seg)], n)


def test_host_copy_of_the_grid_arithmetic_under_the_sanitizers(tmp_path):
    """tools/tile_count_grid_check.cpp: corner adds, both forms of the prefix passes and the decode against a brute-force
    count, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "grid_check")
    r = subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "tile_count_grid_check.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ", 0 mismatches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
