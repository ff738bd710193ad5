"""The occupancy the design rests on and the one recipe libcrt_hip.so is built by, checked without a GPU. hipcc cross-compiles every unit of the
Makefile's HIP_UNITS for gfx950 with -Rpass-analysis=kernel-resource-usage (tools/kernel_resources.py does the same for people; one compile per
unit and process).

The budgets: every kernel family fits what the design promises for it. The plain instantiations of the trace kernel --
crt_trace_kernel<COUNT=false, STAMP=false, SHADOW, TLAS, REFRACT>, the eight a frame without diagnostics can reach, BASELINE's "primary + shadow
ray" configs and the 401-instance scenes included -- must fit 64 VGPRs with no scratch and 5 KiB of LDS: 8 waves per SIMD, 32 per CU;
the opt-in forms beside them and the other families have conditions of their own (FAMILIES below; crt_rays_kernel's: tests/test_trace_rays_cpu.py), which differ on purpose. The register allocator is touchy here (an equivalent
loop-exit test once cost 30 spilled VGPRs), so this is a regression test for the build flags and the code shape, not for the GPU.

The ledger: tests/golden/kernel_resources.json holds, for every unit, every kernel's name and its eight remark fields in the compiler's order
(`python tools/kernel_resources.py --record` writes it). A change that moves a row re-records it and says in its commit message which rows moved
and why; a new kernel appends rows, in whichever unit the code wants it: it needs no translation unit of its own to keep the older rows true.
Rows re-recorded so far: when the BuildBVH kernels were rewritten over shared helpers, two moved, both downwards -- crt_bvh_big_bins
32 -> 30 VGPRs and 57 -> 55 SGPRs, crt_bvh_big_scatter 54 -> 53 SGPRs.

The recipe: the units and the flags are written once, in the Makefile, and everything else that builds or names the library follows it."""
import collections
import glob
import json
import os
import re
import shlex
import shutil
import subprocess

import pytest

from util import HIP_UNITS, kernel_resource_rows, kernel_resources, resource_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LEDGER = os.path.join(ROOT, "tests", "golden", "kernel_resources.json")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")

# unit: the unit whose rows are searched (None: the whole library); prefix: the family is every kernel whose name starts with it; want: how many
# those are, or their sorted names; fits(name, row): the family's budget; total: how many kernels the unit holds; absent: prefixes no kernel of the unit has
Family = collections.namedtuple("Family", "unit prefix want fits total absent", defaults=(None, ()))


def plain_budget(n, r):
    """no scratch, at most 64 VGPRs, no AGPRs, 8 waves per SIMD, the 5 KiB stack in LDS"""
    return r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["AGPRs"] == 0 and r["Occupancy"] == 8 and r["LDS Size"] == 5120


def no_scratch(n, r):
    return r["ScratchSize"] == 0


def gbuffer(n, r):
    if not (r["ScratchSize"] == 0 and r["AGPRs"] == 0 and r["LDS Size"] == 5120):
        return False
    if n == "crt_trace_gbuffer_kernel<true, true, true>":
        # shadow rays + instance tree + refraction at once: bounded at 7 waves/SIMD (DESIGN.md 4c says why), 68 VGPRs
        return r["VGPRs"] == 68 and r["Occupancy"] == 7
    return r["VGPRs"] == 64 and r["Occupancy"] == 8


FAMILIES = {
    # CRT_RENDER_SSAA2 / SSAA4: the supersampled Trace kernel keeps the plain kernels' budget; sixteen instantiations, no more
    "ssaa-plain": Family(None, "crt_trace_ssaa_kernel<false,", 8, plain_budget),
    "ssaa-counted": Family(None, "crt_trace_ssaa_kernel<true,", 8, no_scratch),
    "ssaa": Family(None, "crt_trace_ssaa_kernel<", 16, lambda n, r: True),
    # CRT_RENDER_GBUFFER: eight instantiations (the flag is refused with counters); neither a crt_trace_kernel (eight plain ones: the test
    # below) nor a crt_trace_ssaa_kernel instantiation (sixteen: the row above)
    "gbuffer": Family(None, "crt_trace_gbuffer_kernel<", 8, gbuffer),
    # crt_trace_ao / crt_frame_ao: num, den and the sample counter live across the traversals; the item is loaded again per sample instead of being carried
    "ao": Family("crt_ao.hip", "crt_ao_kernel<", ["crt_ao_kernel<0, false>", "crt_ao_kernel<0, true>", "crt_ao_kernel<1, false>", "crt_ao_kernel<1, true>"], plain_budget, total=5),
    "ao-filter": Family("crt_ao.hip", "crt_ao_filter_kernel", ["crt_ao_filter_kernel"],
                        lambda n, r: r["ScratchSize"] == 0 and r["LDS Size"] == 0 and r["Occupancy"] == 8),
    # the three queries under the inclusive box test: the whole unit, and no second copy of the kernels under upstream's rule in it
    "inclusive": Family("crt_inclusive.hip", "", sorted([f"crt_rays_inclusive_kernel<{x}, {t}>" for x in ("false", "true") for t in ("false", "true")]
                                                       + [f"crt_ao_inclusive_kernel<{x}, {t}>" for x in ("0", "1") for t in ("false", "true")]),
                        plain_budget, absent=("crt_rays_kernel<", "crt_ao_kernel<")),
    # crt_shade_rays: no scratch, no AGPRs, LDS at most 5120 B, 64 VGPRs at 8 waves/SIMD: none of the six needs the bound at 7
    "shade": Family("crt_shade.hip", "", sorted(f"crt_shade_kernel<{w}, {t}>" for w in (1, 2, 3) for t in ("false", "true")),
                    lambda n, r: (r["ScratchSize"] == 0 and r["AGPRs"] == 0 and r["LDS Size"] <= 5120 and r["VGPRs"] <= 64 and r["Occupancy"] == 8
                                  and r.get("VGPRs Spill", 0) == 0)),
}


@needs_hipcc
def test_plain_trace_instantiations_need_no_scratch_and_64_vgprs():
    rows = kernel_resources()
    plain = {k: v for k, v in rows.items() if k.startswith("crt_trace_kernel<false, false,")}
    assert len(plain) == 8, sorted(rows)
    for name, r in plain.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["AGPRs"] == 0 and r["Occupancy"] == 8 and r["LDS Size"] == 5120, (name, r)
    # the instrumented instantiations may use more registers (6 waves/SIMD); the default counted and stamped ones must not spill either
    assert rows["crt_trace_kernel<true, false, false, false, false>"]["ScratchSize"] == 0
    assert rows["crt_trace_kernel<false, true, false, false, false>"]["ScratchSize"] == 0          # the stamped diagnostic launch
    # round 5: the refill kernel met the gate it was given (64 VGPRs, no scratch, occupancy 8) -- its loss is not a register artefact;
    # the wavefront form's two kernels run at the default kernel's occupancy too
    r = rows["crt_trace_refill_kernel<false, false>"]
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8 and r["LDS Size"] == 5120, r
    for name in ("crt_primary_kernel<false>", "crt_bounce_kernel<false>"):
        assert rows[name]["ScratchSize"] == 0 and rows[name]["VGPRs"] <= 64 and rows[name]["Occupancy"] == 8, (name, rows[name])
    # the block form keeps occupancy 8 at the price of a small spill (7 VGPRs = 32 B of scratch per lane, stated in DESIGN.md 4f: its 0.81x is
    # measured WITH that spill)
    r = rows["crt_trace_block_kernel<false, false>"]
    assert r["VGPRs"] <= 64 and r["Occupancy"] == 8 and r["ScratchSize"] <= 32, r
    # round 6: the LDS-staged tree tops -- four waves per workgroup, 15.75 KiB table + 4 x 3.75 KiB of stack = 30.75 KiB -> five workgroups per CU
    r = rows["crt_trace_ldstop_kernel<false>"]
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 96 and r["Occupancy"] == 5 and r["LDS Size"] == 252 * 64 + 4 * 15 * 256, r


@needs_hipcc
@pytest.mark.parametrize("family", list(FAMILIES))
def test_kernel_family_fits_its_budget(family):
    f = FAMILIES[family]
    rows = kernel_resources() if f.unit is None else dict(kernel_resource_rows(source=f.unit))
    found = {n: r for n, r in rows.items() if n.startswith(f.prefix)}
    for n, r in sorted(found.items()):
        print(resource_line(n, r))
    assert (len(found) if isinstance(f.want, int) else sorted(found)) == f.want, sorted(rows)
    for n, r in found.items():
        assert f.fits(n, r), resource_line(n, r)
    assert f.total is None or len(rows) == f.total, sorted(rows)
    assert not [n for n in rows if n.startswith(f.absent)]


@needs_hipcc
@pytest.mark.parametrize("unit", HIP_UNITS)
def test_every_kernel_keeps_its_recorded_resources(unit):
    ledger = json.load(open(LEDGER))
    assert list(ledger) == list(HIP_UNITS)
    want = ledger[unit]
    got = [[n, r] for n, r in kernel_resource_rows(source=unit)]
    names, recorded = [n for n, _ in got], [n for n, _ in want]
    assert names == recorded, (f"the kernel list of {unit} changed: added {[n for n in names if n not in recorded]}, removed {[n for n in recorded if n not in names]}, "
                               f"or reordered -- record it again (tools/kernel_resources.py --record) and say so in the commit message")
    moved = [f"recorded {resource_line(n, w)} SGPR spill {w.get('SGPRs Spill', -1)}\ncompiled {resource_line(n, g)} SGPR spill {g.get('SGPRs Spill', -1)}"
             for (n, g), (_, w) in zip(got, want) if g != w]
    assert not moved, f"{len(moved)} of {unit}'s {len(got)} rows moved:\n" + "\n".join(moved)


def link_line(*make_args):
    """the tokens of the one compiler line that `make -n` prints for the library when crt_shim.hip counts as new"""
    p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/csrc/crt_shim.hip", *make_args], cwd=ROOT, stdout=subprocess.PIPE, text=True, check=True)
    lines = [l for l in p.stdout.splitlines() if "-shared" in l.split()]
    assert len(lines) == 1, p.stdout
    return shlex.split(lines[0])


@pytest.mark.skipif(shutil.which("make") is None, reason="needs make")
def test_the_library_has_one_build_recipe(tmp_path):
    """A library without one of the units links but cannot be loaded (crt_query_host.h, crt_ao_host.h, crt_shade_host.h and crt_frame.h refer to
    their kernels), and an A/B library built with other flags than the Makefile's measures something else than what ships."""
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    units = re.search(r"^HIP_UNITS = (.*)$", makefile, re.M).group(1).split()
    flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    paths = ["clraytracer_amd/csrc/" + u for u in units]
    # no unit forgotten in either direction; the tool reads the same list
    assert sorted(units) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "clraytracer_amd", "csrc", "*.hip"))) and units[0] == "crt_shim.hip"
    assert list(HIP_UNITS) == units
    # the rule: compiler, HIPFLAGS, -shared -o <library>, the units in order, nothing else ...
    assert link_line("clraytracer_amd/csrc/libcrt_hip.so")[1:] == flags + ["-shared", "-o", "clraytracer_amd/csrc/libcrt_hip.so"] + paths
    # ... and the A/B tools' way through it: their output path, their flags behind the Makefile's
    variant = str(tmp_path / "libcrt_hip.so.tmp")
    assert link_line(f"HIP_SO={variant}", "EXTRA_HIPFLAGS=-DCRT_RECIPE_PROBE=1", variant)[1:] == flags + ["-DCRT_RECIPE_PROBE=1", "-shared", "-o", variant] + paths
    for tool in ("ab_build.sh", "ab_define.sh"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert "EXTRA_HIPFLAGS" in text and ".hip" not in text and "--offload-arch" not in text, tool
    # the command for integrators who do not use make
    doc = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if "hipcc" in l and "-shared" in l]
    assert len(doc) == 1
    assert "--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC" in doc[0] and " ".join(paths) in doc[0]
    # crt_shim.hip's header names every unit beside it
    head = open(os.path.join(ROOT, "clraytracer_amd", "csrc", "crt_shim.hip")).read().split("#include")[0]
    assert all(u in head for u in units[1:]), head
