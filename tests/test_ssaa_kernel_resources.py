"""CRT_RENDER_SSAA2 / SSAA4 without a GPU: the supersampled Trace kernel keeps the occupancy the design rests on (hipcc cross-compiles
crt_shim.hip for gfx950 with -Rpass-analysis=kernel-resource-usage, as test_kernel_resources does), the flags have their ABI values
and the C wrapper of Renderer::SetSupersampling is bound."""
import os
import re
import shutil

import pytest

from util import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_ssaa_instantiations_fit_the_plain_kernels_budget():
    rows = kernel_resources()
    plain = {k: v for k, v in rows.items() if k.startswith("crt_trace_ssaa_kernel<false,")}
    counted = {k: v for k, v in rows.items() if k.startswith("crt_trace_ssaa_kernel<true,")}
    assert len(plain) == 8 and len(counted) == 8, sorted(rows)
    for name, r in plain.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["AGPRs"] == 0 and r["Occupancy"] == 8 and r["LDS Size"] == 5120, (name, r)
    for name, r in counted.items():
        assert r["ScratchSize"] == 0, (name, r)


def test_ssaa_flags_and_binding():
    api = open(os.path.join(ROOT, "include/crt_api.h")).read()
    assert re.search(r"CRT_RENDER_SSAA2\s*=\s*2048\b", api)
    assert re.search(r"CRT_RENDER_SSAA4\s*=\s*4096\b", api)
    assert "void crth_set_supersampling(int factor);" in open(os.path.join(ROOT, "include/crt_host.h")).read()
    from clraytracer_amd import _lib
    assert "crth_set_supersampling" in _lib.HOST_API
