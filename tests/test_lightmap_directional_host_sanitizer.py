"""CPU: directional lightmaps' host side under AddressSanitizer + UBSan: the stand-alone driver of `make -C path_tracer_amd/csrc host-asan`
in its mode `lightmaps_dir <n> <seed>` makes gradients with lm_gradient (pt_lightmap.h) from random first-moment sums, denormal ones and
zero normals among them, in tables that fill their allocation exactly, and runs lightmap_lookup_directional (pt_materials.h, the function the
kernels run) under a normal texture at random hits whose UVs are far outside [0, 1], huge, mirrored and overflowing: no texel index leaves its
map or its gradient, and no result is negative or a NaN.  Any sanitizer report fails the test."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "path_tracer_amd", "csrc")
EXE = os.path.join(ROOT, "path_tracer_amd", "host_sanitize")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-C", CSRC, "host-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return EXE


@pytest.mark.parametrize("n, seed", [(1, 1), (60, 7), (600, 11), (601, 12)])
def test_directional_lookup_under_asan_and_ubsan(exe, n, seed):
    r = subprocess.run([exe, "lightmaps_dir", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["triangles"] == n and res["lookups"] > n and res["checksum"] > 0.0 and (n == 1 or res["moved"] > n)
    again = subprocess.run([exe, "lightmaps_dir", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert again.stdout == r.stdout                                              # deterministic: nothing uninitialised is read
