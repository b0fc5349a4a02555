"""CPU: the reflection probes' host side under AddressSanitizer + UBSan: the stand-alone driver of `make -C path_tracer_amd/csrc host-asan` in
its mode `proberadiance <n> <seed>` builds random grids, axes of a single node among them, prefilters random raw radiance maps with empty
texels (map sides 2..16, 1..8 levels) through probe_prefilter_texel into a table that fills its allocation exactly, and runs
probe_grid_specular (pt_probe.h, the function the kernels run), with a random depth table and without, at points inside, far outside, huge,
infinite and NaN, with zero, huge, infinite and NaN directions and alphas: whatever the query is, no texel leaves its node's map, no level the
levels and no node index the grid.  The same built program as tests/test_probe_depth_host_sanitizer.py, run as a process, with nothing
preloaded.  Any sanitizer report fails the test."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "path_tracer_amd", "csrc")
EXE = os.path.join(ROOT, "path_tracer_amd", "host_sanitize")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
GRIDS = 6


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-C", CSRC, "host-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return EXE


@pytest.mark.parametrize("n, seed", [(1, 1), (64, 7), (800, 11), (801, 12)])
def test_prefilter_and_specular_lookup_under_asan_and_ubsan(exe, n, seed):
    r = subprocess.run([exe, "proberadiance", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["lookups"] == GRIDS * n and 0 < res["lit"] <= res["lookups"]
    assert res["round_trip"] == 1 and res["finite"] == 1 and res["filtered"] > 0.0
    if n >= 64:
        assert res["lit"] < res["lookups"] and res["checksum"] > 0.0              # occluded and invalid corners leave some points unlit
    again = subprocess.run([exe, "proberadiance", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert again.stdout == r.stdout                                              # deterministic: nothing uninitialised is read
