"""What one walk step of blend_kernel issues, read from the gfx950 assembly (no GPU needed: hipcc cross-compiles, with the
flags of gaussreg_amd/build.py and tools/kernel_resources.py).  The walk loop holds the four ds_read_b128 of a step's two
records and, unlike the batch loop around it, no barrier; it runs from the first label a branch jumps back to (the compiler
lays the latch blocks out in front of the header) to the last such branch.
    python tools/blend_walk_isa.py [rasterizer.hip]        (DESIGN.md 3.3 quotes its output)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
BRANCH = re.compile(r"s_(?:c?branch\w*|setpc_b64)")


def walk_loops(asm):
    """{kernel name: instruction lines of its walk loop} for every blend_kernel instance in `asm`."""
    out = {}
    for m in re.finditer(r"^(_Z\w*blend_kernel\w*):[^\n]*\n(.*?)^\s*s_endpgm", asm, re.S | re.M):
        lines = [l.split(";")[0].strip() for l in m.group(2).splitlines()]
        lines = [l for l in lines if l and not l.startswith(".") or re.match(r"\.LBB\w+:", l)]
        label = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
        last_back_edge = {}
        for j, l in enumerate(lines):
            t = l.split()
            if BRANCH.match(t[0]) and t[-1] in label and label[t[-1]] < j:
                last_back_edge[label[t[-1]]] = j
        loops = [lines[i + 1:j + 1] for i, j in last_back_edge.items()]
        loops = [b for b in loops if sum(l.startswith("ds_read_b128") for l in b) >= 4 and "s_barrier" not in b]
        assert loops, m.group(1)
        out[m.group(1)] = max(loops, key=len)
    return out


def classify(body):
    c = {"valu": 0, "salu": 0, "lds": 0, "waitcnt": 0, "nop": 0, "branch": 0, "other": 0, "label": 0}
    for l in body:
        op = l.split()[0]
        if l.endswith(":"):
            c["label"] += 1
        elif op == "s_nop":
            c["nop"] += 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif BRANCH.match(op):
            c["branch"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        else:
            c["other"] += 1
    c["total"] = sum(v for k, v in c.items() if k != "label")
    return c


def main():
    src = os.path.join(ROOT, "gaussreg_amd", "csrc", sys.argv[1] if len(sys.argv) > 1 else "rasterizer.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rasterizer.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        loops = walk_loops(open(out).read())
    for name, body in sorted(loops.items()):
        # blend_kernel<FAST_EXP, KEEP, AUX>: the template arguments are mangled as Lb0E / Lb1E in that order
        args = re.search(r"blend_kernelILb([01])ELb([01])ELb([01])EE", name).groups()
        print("blend_kernel<%s>" % ", ".join("true" if a == "1" else "false" for a in args),
              " ".join(f"{k}={v}" for k, v in classify(body).items()))


if __name__ == "__main__":
    main()
