"""CPU: roughness maps' host side under AddressSanitizer + UBSan: the stand-alone driver of `make -C path_tracer_amd/csrc host-asan` in its
mode `roughness <n> <seed>` goes through the setter's refusals (kinds that are not GGX, bad material and texture indices: each changes
nothing), puts a 5 x 3 map on n random triangles with mirrored, negative, exactly-1 and 1e6 UVs, a 1 x 1 map on a model without UVs and an
8 x 4 map on a third, and runs surface_alpha (pt_materials.h, the function the kernels run) at random hits, vertices and edges among them.
Every map's values lie in a range of its own, so whatever the UVs are no texel leaves its texture: neither the allocation (the sanitizer)
nor the map (the driver's own check).  Clearing the maps must give the bytes of the scene that never had one.  The same built program as
tests/test_probe_radiance_host_sanitizer.py, run as a process, with nothing preloaded.  Any sanitizer report fails the test."""
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


@pytest.mark.parametrize("n, seed", [(1, 1), (5, 3), (500, 7), (801, 12)])
def test_setter_and_surface_alpha_under_asan_and_ubsan(exe, n, seed):
    r = subprocess.run([exe, "roughness", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["triangles"] == n and res["refused"] == 11 and res["checksum"] > 0.0, res
    assert all(h > 0 for h in res["hits"]) and sum(res["hits"]) <= 4 * n + 64, res          # every map was read
    again = subprocess.run([exe, "roughness", str(n), str(seed)], capture_output=True, text=True, env=ENV, timeout=600)
    assert again.stdout == r.stdout                                              # deterministic: nothing uninitialised is read
