"""CPU: the census table (tests/variant_census_common.py) against the library's own enumeration of the kernels its keyed launchers compile
(pt_variant_axes, pt_variant_compiled: the bounds and the predicates the launchers instantiate from).  Every compiled variant belongs to the
set of some case, and no case names a point that is no kernel: a new axis value, or a new point of a predicate, needs a row in the table, and
a row cannot be dropped while its variants exist.  No device is touched."""
import itertools
import re

import pytest

from conftest import ROOT
from variant_census_common import CASES, LAUNCHERS, table_variants


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def test_the_launchers_are_the_headers(api):
    """the table's launcher names, the binding's and include/pt_api.h's pt_launcher are one list"""
    hdr = open(f"{ROOT}/include/pt_api.h").read()
    enum = re.search(r"typedef enum pt_launcher \{(.*?)\} pt_launcher;", hdr, re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",")]
    assert names[-1] == "PT_LAUNCHER_COUNT"
    assert tuple(n[len("PT_LAUNCHER_"):].lower() for n in names[:-1]) == api.LAUNCHERS == LAUNCHERS
    import ctypes
    import numpy as np
    b = np.zeros(6, np.uint32)
    assert api.lib().pt_variant_axes(len(LAUNCHERS), b.ctypes.data_as(ctypes.c_void_p)) < 0, "a launcher past the last"
    assert not api.lib().pt_variant_compiled(len(LAUNCHERS), b.ctypes.data_as(ctypes.c_void_p))


@pytest.mark.parametrize("launcher", LAUNCHERS)
def test_every_compiled_variant_has_a_case(api, launcher):
    """the union of the cases' sets IS the launcher's compiled set: zero compiled variants without a case, zero cases on a point that is no kernel"""
    compiled = api.compiled_variants(launcher)
    assert compiled, launcher
    table = {v for v in table_variants() if v[0] == launcher}
    assert not compiled - table, f"compiled {launcher} variants that no case launches: {sorted(compiled - table)}"
    assert not table - compiled, f"cases expect {launcher} variants the library does not compile: {sorted(table - compiled)}"


def test_a_point_outside_the_bounds_is_no_kernel(api):
    for launcher in LAUNCHERS:
        bounds = api.variant_axes(launcher)
        assert 1 <= len(bounds) <= 6 and all(b >= 1 for b in bounds)
        for k in range(len(bounds)):
            p = [0] * len(bounds)
            p[k] = bounds[k]
            assert not api.variant_compiled(launcher, p), (launcher, p)
    # the surface pass has no kernel for the terminal queue, and an inline shadow walk only in the untextured Lambertian pass without media
    assert not api.variant_compiled("shade", (0, 0, 0, 0, 0, 0))
    assert api.variant_compiled("shade", (1, 0, 1, 0, 0, 0)) and not api.variant_compiled("shade", (4, 0, 1, 0, 0, 0))
    assert not api.variant_compiled("shade", (1, 1, 1, 0, 0, 0)) and not api.variant_compiled("shade", (1, 0, 2, 0, 0, 1))


def test_the_counts(api):
    """DESIGN.md's figures"""
    counts = {launcher: len(api.compiled_variants(launcher)) for launcher in LAUNCHERS}
    assert counts == {"shade": 336, "terminal": 4, "closest": 48, "any": 16, "fused": 4, "generate": 8, "guide_rays": 4, "accumulate": 12}, counts
    grid = sum(len(list(itertools.product(*[range(n) for n in api.variant_axes(launcher)]))) for launcher in LAUNCHERS)
    assert grid > sum(counts.values())
    assert len(CASES) == 129


def test_the_rows_that_alone_launch_a_variant():
    """89 of the 129 rows are the only case of some variant (dropping one loses it from the union above); the others run the same kernels by
    another route (an adaptive case's first round is a rectangle render) or on a room the census wants as well, so the row count is held
    too: no row leaves the table unnoticed"""
    owners = {}
    for c in CASES:
        for v in c.variants():
            owners.setdefault(v, []).append(c.id)
    sole = {ids[0] for ids in owners.values() if len(ids) == 1}
    for cid in sole:
        rest = [c for c in CASES if c.id != cid]
        assert table_variants(rest) != table_variants(), cid
    assert len(sole) == 89, len(sole)
