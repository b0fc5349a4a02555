"""CPU: the host side of direct light sampled at the texel under AddressSanitizer + UBSan: the stand-alone driver of
`make -C path_tracer_amd/csrc host-asan` in its mode `lightmap_direct <n> <seed>` runs lm_light_sample (pt_lightmap.h, the function the
kernels run) and the host fold of X = G + D over random texels and designed ones - a light point exactly at the origin, cosl == 0, a
zero-area light triangle, a draw past the cdf's last entry, x == 1.0 - against light tables that fill their allocations exactly: no index
leaves its table, and no D is negative, a NaN or longer than 100.  Any sanitizer report fails the test."""
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
def test_light_sample_and_fold_under_asan_and_ubsan(exe, n, seed):
    r = subprocess.run([exe, "lightmap_direct", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["texels"] == n + 4 and res["samples"] == 4 * n + 4 * 64 and res["lights"] == 4 + n % 7
    # the designed cases were met: the draw of exactly 1.0 ran past the cdf's end onto the last entry, the grazing texel cast rays that add
    # nothing, the texel at the zero-area triangle's point picked it; and the ordinary samples add light
    # (with n odd the zero-area triangle has the weight 0 its area gives it, and nothing picks it)
    assert res["last_entry"] >= 1 and res["grazing"] >= 1 and res["zero_area"] >= res["at_origin"] and (res["at_origin"] >= 1) == (n % 2 == 0)
    assert 0 < res["cast"] < res["samples"] and res["checksum"] > 0.0
    again = subprocess.run([exe, "lightmap_direct", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert again.stdout == r.stdout                                              # deterministic: nothing uninitialised is read
