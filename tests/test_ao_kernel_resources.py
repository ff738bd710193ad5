"""The resources of the ambient-occlusion kernels (crt_ao.hip, the third unit of libcrt_hip.so), checked without a GPU as
tests/test_kernel_resources.py checks the Trace kernels: every crt_ao_kernel<SOURCE, TLAS> fits the plain kernels' budget -- no scratch, at
most 64 VGPRs, 8 waves per SIMD, the 5 KiB stack in LDS (num, den and the sample counter live across the traversals; the item is loaded
again per sample instead of being carried) -- and the kernels of the two older units are the ones they were: their names, in the compiler's
order, and their figures equal the listing recorded before the unit was added (tests/golden/kernel_resources_before_ao.json)."""
import json
import os
import shutil

import pytest

from util import kernel_resource_rows, resource_line

HIPCC = "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_resources_before_ao.json")
FIELDS = ("VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS Size")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_hipcc
def test_every_ao_kernel_fits_the_plain_kernels_budget():
    rows = dict(kernel_resource_rows(source="crt_ao.hip"))
    for n, r in sorted(rows.items()):
        print(resource_line(n, r))
    ao = {n: r for n, r in rows.items() if n.startswith("crt_ao_kernel<")}
    assert sorted(ao) == ["crt_ao_kernel<0, false>", "crt_ao_kernel<0, true>", "crt_ao_kernel<1, false>", "crt_ao_kernel<1, true>"]
    for n, r in ao.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["AGPRs"] == 0 and r["Occupancy"] == 8 and r["LDS Size"] == 5120, resource_line(n, r)
    r = rows["crt_ao_filter_kernel"]
    assert r["ScratchSize"] == 0 and r["LDS Size"] == 0 and r["Occupancy"] == 8, resource_line("crt_ao_filter_kernel", r)
    assert len(rows) == 5


@needs_hipcc
@pytest.mark.parametrize("source", ["crt_shim.hip", "crt_rays.hip"])
def test_the_older_units_kernels_are_unchanged(source):
    want = json.load(open(GOLDEN))[source]
    got = [[n, {f: r.get(f) for f in FIELDS}] for n, r in kernel_resource_rows(source=source)]
    assert [n for n, _ in got] == [n for n, _ in want]
    assert got == want
