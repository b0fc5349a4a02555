"""CPU: the a-trous core of pt_filter.h (spatial_variance, atrous_level: the functions every filter kernel runs) under AddressSanitizer +
UBSan: the stand-alone driver of `make -C path_tracer_amd/csrc host-asan` in its mode `screenfilter <seed>` runs the screen rule on random
images of 1 x 1, 5 x 3, 16 x 16 and 37 x 19 pixels with miss pixels, invalid pixels and two models, through the 7 x 7 variance and 8 levels,
where step 128 leaves every map: no tap index leaves its image.  The driver then checks the neighbour rules' defining property itself: with
one model, every pixel a valid hit and no reach, the texel rule gives the screen rule's bits (exit 7 if not).  Any sanitizer report fails the
test."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "path_tracer_amd", "csrc")
EXE = os.path.join(ROOT, "path_tracer_amd", "host_sanitize")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
PIXELS = 1 + 5 * 3 + 16 * 16 + 37 * 19


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-C", CSRC, "host-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return EXE


@pytest.mark.parametrize("seed", [1, 3, 7])
def test_screen_filter_under_asan_and_ubsan(exe, seed):
    r = subprocess.run([exe, "screenfilter", str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split("\n")[-1])
    # (colour | variance) of every pixel, under the screen rule on the hostile images and once for the two rules' common result
    assert res["pixels"] == PIXELS and res["finite"] == PIXELS * 4 * 2 and res["checksum"] > 0.0
    again = subprocess.run([exe, "screenfilter", str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert again.stdout == r.stdout                                              # deterministic: nothing uninitialised is read
