#!/usr/bin/env python3
"""Compile the translation units of libcrt_hip.so (the Makefile's HIP_UNITS, with its HIPFLAGS) for gfx950 with -Rpass-analysis=kernel-resource-usage and print one
line per kernel: VGPRs, AGPRs, scratch bytes per lane, occupancy, LDS bytes. Runs without a GPU (hipcc cross-compiles).

    python tools/kernel_resources.py [filter-substring] [-D...]
    python tools/kernel_resources.py --record        writes tests/golden/kernel_resources.json, the ledger tests/test_kernel_resources.py compares with

The tests read the same figures through kernel_resources() / kernel_resource_rows() (tests/util.py imports this file by path): one compile per unit and process.
"""
import functools
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LEDGER = os.path.join(ROOT, "tests", "golden", "kernel_resources.json")


def makefile_words(variable):
    """the words of the Makefile's `variable = ...` line, $(ARCH) expanded"""
    value = re.search(rf"^{variable} = (.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1)
    return value.replace("$(ARCH)", "gfx950").split()


HIP_UNITS = tuple(makefile_words("HIP_UNITS"))     # the units of libcrt_hip.so, in link order


def kernel_resource_rows(defs=(), source=HIP_UNITS[0]):
    """[(demangled kernel name, {remark field: int})] of one unit (default: crt_shim.hip) built with the Makefile's HIPFLAGS (+ defs), one entry per
    remark block in the compiler's order. (The two kernels in an anonymous namespace both demangle to the empty name here: a list keeps both.)"""
    return _compile(tuple(defs), source)


@functools.lru_cache(maxsize=None)
def _compile(defs, source):
    cmd = [HIPCC] + makefile_words("HIPFLAGS") + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "clraytracer_amd/csrc", source), "-o", os.devnull] + list(defs)
    p = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode:
        raise RuntimeError(f"hipcc failed ({p.returncode}):\n{p.stderr[-2000:]}")
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip()
            cur = {}
            rows.append((re.sub(r"\(.*", "", name).replace("void ", ""), cur))
            continue
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def kernel_resources(defs=()):
    """{demangled kernel name: {remark field: int}} of every unit of the library, over the same (memoised) compiles."""
    rows = {}
    for source in HIP_UNITS:
        for name, r in kernel_resource_rows(defs, source):
            rows.setdefault(name, {}).update(r)
    return rows


def resource_line(name, r):
    return (f"{name:70s} VGPR {r.get('VGPRs', -1):3d} AGPR {r.get('AGPRs', -1):3d} scratch {r.get('ScratchSize', -1):4d} occ {r.get('Occupancy', -1):2d} "
            f"LDS {r.get('LDS Size', -1):6d} SGPR {r.get('TotalSGPRs', -1):3d} spillV {r.get('VGPRs Spill', -1):3d}")


def record():
    """{unit: [[kernel name, {remark field: int}], ...]} of every unit into LEDGER: one row per line, fields in the compiler's order, so a re-record diffs row by row"""
    units = []
    for source in HIP_UNITS:
        rows = ",\n".join("  " + json.dumps([name, r]) for name, r in kernel_resource_rows(source=source))
        units.append(f" {json.dumps(source)}: [\n{rows}\n ]")
    with open(LEDGER, "w") as f:
        f.write("{\n" + ",\n".join(units) + "\n}\n")


def main():
    flt = [a for a in sys.argv[1:] if not a.startswith("-")]
    defs = [a for a in sys.argv[1:] if a.startswith("-")]
    try:
        if defs == ["--record"] and not flt:
            return record()
        rows = [row for source in HIP_UNITS for row in kernel_resource_rows(defs, source)]
    except RuntimeError as e:
        sys.stderr.write(str(e) + "\n")
        raise SystemExit(1)
    for name, r in rows:
        if not flt or any(f in name for f in flt):
            print(resource_line(name, r))


if __name__ == "__main__":
    main()
