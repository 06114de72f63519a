"""Compiler resource remarks of the rasterizer kernels the depth / alpha maps touch (no GPU needed: hipcc cross-compiles for
gfx950).  The colour-only instances keep the figures they had before the maps existed; the new instances have no scratch
and keep the workgroups per CU that DESIGN.md 3.3 states for them."""
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LDS_PER_CU = 160 * 1024
BLEND_AUX_WGS_PER_CU = 8
RENDER_BWD_AUX_WGS_PER_CU = 3


def _resources(src, pattern):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), src, pattern],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"\s*(\w+<[^>]*>)\s+(.*)", line)
        if m:
            rows[m.group(1)] = {k.strip(): int(v) for k, v in re.findall(r"([A-Za-z ]+)=(\d+)", m.group(2))}
    return rows


def _args(name):
    return [a.strip() for a in name[name.index("<") + 1:-1].split(",")]


def _no_scratch(name, v):
    assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (name, v)


def test_blend_instances():
    rows = _resources("rasterizer.hip", "blend_kernel")
    colour = {k: v for k, v in rows.items() if len(_args(k)) == 2 or _args(k)[2] == "false"}
    aux = {k: v for k, v in rows.items() if k not in colour}
    assert len(colour) == 4 and len(aux) == 4, sorted(rows)
    for name, v in colour.items():
        assert v["VGPRs"] == 64 and v["Occupancy"] == 8 and v["LDS Size"] == 19328, (name, v)
        _no_scratch(name, v)
    assert sorted(tuple(_args(k)[:2]) for k in aux) == sorted((a, b) for a in ("false", "true") for b in ("false", "true"))
    for name, v in aux.items():
        _no_scratch(name, v)
        assert BLEND_AUX_WGS_PER_CU * v["LDS Size"] <= LDS_PER_CU, (name, v)
        assert v["Occupancy"] >= BLEND_AUX_WGS_PER_CU * 4 // 4, (name, v)  # 4 waves per workgroup over 4 SIMDs


def test_backward_instances():
    rows = _resources("rasterizer_backward.hip", "backward_kernel")
    render = {k: v for k, v in rows.items() if k.startswith("render_backward_kernel")}
    pre = {k: v for k, v in rows.items() if k.startswith("preprocess_backward_kernel")}
    assert len(render) == 4 and len(pre) == 8, sorted(rows)
    for name, v in rows.items():
        _no_scratch(name, v)
    for name, v in render.items():
        a = _args(name)
        if len(a) == 1 or a[1] == "false":
            assert v["LDS Size"] == 50704, (name, v)
        else:
            assert RENDER_BWD_AUX_WGS_PER_CU * v["LDS Size"] <= LDS_PER_CU, (name, v)
            # a safety margin, not a hardware figure: with 54 032 bytes only two workgroups were resident on the device
            # although 3 x 54 032 < 160 KiB.  The allocation block size was not measured (1 280 bytes or
            # 2 KiB both explain the observation); rounding up to 2 KiB is the stricter of the two guesses.
            assert RENDER_BWD_AUX_WGS_PER_CU * (-(-v["LDS Size"] // 2048) * 2048) <= LDS_PER_CU, (name, v)
            assert v["Occupancy"] >= RENDER_BWD_AUX_WGS_PER_CU, (name, v)
