"""CPU: the texel filter's host side under AddressSanitizer + UBSan: the stand-alone driver of `make -C path_tracer_amd/csrc host-asan` in its
mode `texelfilter <n> <seed>` builds the texel tables of random triangles with hostile UVs (far outside [0, 1], huge, mirrored, overflowing,
a triangle of no area) on maps from 1 x 1 up, sides that are no multiple of 16 among them, and runs the whole filter of pt_lightmap_filter.h
(the functions the kernels run) with 8 levels, where step 128 exceeds every map: no tap index leaves its map.  Any sanitizer report fails
the test."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "path_tracer_amd", "csrc")
EXE = os.path.join(ROOT, "path_tracer_amd", "host_sanitize")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
TEXELS = 1 + 5 * 3 + 16 * 16 + 37 * 19 + 2 * 37 + 48 * 32


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-C", CSRC, "host-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return EXE


@pytest.mark.parametrize("n, seed", [(1, 1), (7, 3), (60, 7)])
def test_texel_filter_under_asan_and_ubsan(exe, n, seed):
    r = subprocess.run([exe, "texelfilter", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["triangles"] == n and 0 < res["covered"] <= TEXELS and res["finite"] == TEXELS * 3 * 6 and res["checksum"] > 0.0
    again = subprocess.run([exe, "texelfilter", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert again.stdout == r.stdout                                              # deterministic: nothing uninitialised is read
