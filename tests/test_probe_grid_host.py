"""CPU: the irradiance volume (pt_set_probe_grid, pt_get_probe_grid_info, pt_probe_grid_lookup, pt_probe_backfaces) without a GPU: the symbols,
every refusal include/pt_api.h promises before any device call and their order, each with "nothing changed" checked, the host evaluation of
the lookup against the numpy restatement of tests/probe_grid_common.py bit for bit, its exact cases, validity, the clamp, the unit convention
and the grid's lifetime.  No GPU is touched (the device lookup, the view and the census: tests/test_gpu_probe_grid.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import lightmap_common as LC
import probe_grid_common as PG
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, STATE, LIMIT = -1, -3, -5
NEW_SYMBOLS = ["pt_set_probe_grid", "pt_get_probe_grid_info", "pt_probe_grid_lookup", "pt_probe_backfaces"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _renderer(api):
    sc, _ = LC.cornell_atlas_scene()
    return api.Renderer(sc, 48, 32), sc


def _grid_struct(api, origin=(0, 0, 0), cell=(1, 1, 1), count=(2, 2, 2), bias=0.0, reserved=(0, 0, 0, 0)):
    return api.ProbeGrid((C.c_float * 3)(*origin), (C.c_float * 3)(*cell), (C.c_uint32 * 3)(*count), bias, (C.c_uint32 * 4)(*reserved))


def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert "typedef struct pt_probe_grid" in header and C.sizeof(api.ProbeGrid) == 56
    methods = ("set_probe_grid", "set_probe_grid_sums", "probe_grid_info", "probe_grid_lookup", "probe_backfaces", "probe_validity", "bake_probe_grid")
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for method in methods:
        assert callable(getattr(api.Renderer, method))
        assert method + "(" in wrapper, method
    assert "probes as the fallback of unmapped surfaces" not in header


def test_refusals_and_their_order_change_nothing(api):
    r, _ = _renderer(api)
    g = PG.random_grid((3, 2, 4), 5, invalid=0.2, bias=0.25)
    g.set_on(r)
    P, n = PG.query_points(g, 64, 6)
    before, info, scene = r.probe_grid_lookup(P, n), r.probe_grid_info(), r.scene_info().as_dict()
    assert info[2] == (3, 2, 4) and info[3] == 0.25 and info[4] == int(g.valid.sum()) < 24
    L = r.L
    sh = np.ones((8, 9, 3), F)
    one = np.zeros(27, F)            # never read past the counts: each of these is refused before a coefficient is

    def bad(value):
        a = sh.copy()
        a[5, 8, 1] = value
        return a
    nan, inf = float("nan"), float("inf")
    refusals = [
        (None, sh, ARG),
        (dict(reserved=(0, 0, 1, 0)), sh, ARG),
        (dict(), None, ARG), (dict(count=(0, 2, 2)), sh, ARG), (dict(count=(2, 0, 2)), sh, ARG), (dict(count=(2, 2, 0)), sh, ARG),
        (dict(count=(0, 0, 0)), sh, ARG), (dict(count=(2, 0, 0)), None, ARG),
        (dict(count=(257, 1, 1)), one, LIMIT), (dict(count=(1, 257, 1)), one, LIMIT), (dict(count=(1, 1, 257)), one, LIMIT),
        (dict(origin=(nan, 0, 0)), sh, ARG), (dict(origin=(0, inf, 0)), sh, ARG), (dict(cell=(0, 1, 1)), sh, ARG), (dict(cell=(1, -1, 1)), sh, ARG),
        (dict(cell=(1, 1, nan)), sh, ARG), (dict(cell=(inf, 1, 1)), sh, ARG), (dict(bias=-0.5), sh, ARG), (dict(bias=nan), sh, ARG),
        (dict(bias=inf), sh, ARG),
        (dict(), bad(nan), ARG), (dict(), bad(inf), ARG), (dict(), bad(-inf), ARG),
        # where several apply: g, the reserved words, the pointer against the counts, the limit, the fields, the coefficients last
        (dict(reserved=(1, 0, 0, 0), count=(257, 1, 1)), one, ARG), (dict(count=(257, 0, 1)), one, ARG),
        (dict(count=(257, 1, 1), cell=(0, 1, 1)), one, LIMIT), (dict(cell=(0, 1, 1)), bad(nan), ARG),
    ]
    for kw, coeff, code in refusals:
        gs = None if kw is None else C.byref(_grid_struct(api, **kw))
        assert L.pt_set_probe_grid(r.ctx, gs, _p(coeff), None) == code, (kw, code)
        now = r.probe_grid_info()
        assert now[2:] == info[2:] and np.array_equal(now[0], info[0]) and np.array_equal(now[1], info[1]) and r.scene_info().as_dict() == scene
        after = r.probe_grid_lookup(P, n)
        assert_bit_equal(after[0], before[0], f"lookup after the refused call {kw}")
        assert np.array_equal(after[1], before[1])
    # the lookup's own refusals
    out = np.zeros((4, 3), F); lit = np.zeros(4, np.uint8)
    assert L.pt_probe_grid_lookup(r.ctx, 0, 4, None, _p(n), _p(out), _p(lit)) == ARG
    assert L.pt_probe_grid_lookup(r.ctx, 0, 4, _p(P), _p(n), _p(out), None) == ARG
    assert L.pt_probe_grid_lookup(r.ctx, 0, 0, None, None, None, None) == 0
    # negative coefficients are legal, and setting or clearing moves neither the build nor the flattened scene
    assert L.pt_set_probe_grid(r.ctx, C.byref(_grid_struct(api)), _p(-sh), None) == 0
    assert r.probe_grid_info()[2] == (2, 2, 2) and r.probe_grid_info()[4] == 8 and r.scene_info().as_dict() == scene
    r.set_probe_grid(None, None, None)
    assert r.probe_grid_info()[2] == (0, 0, 0) and r.probe_grid_info()[4] == 0 and r.scene_info().as_dict() == scene
    r.set_probe_grid(None, None, None)                                            # clearing what is not there is fine
    assert L.pt_probe_grid_lookup(r.ctx, 0, 4, _p(P), _p(n), _p(out), _p(lit)) == STATE
    assert L.pt_probe_grid_lookup(r.ctx, 1, 4, _p(P), _p(n), _p(out), _p(lit)) == STATE      # before any device call


def test_census_refusals_are_those_of_the_probe_bake(api):
    r, _ = _renderer(api)
    L = r.L
    pos = np.zeros((2, 3), F); hits = np.zeros(2, np.uint32); back = np.zeros(2, np.uint32)
    good = api.ProbeParams(0, 4, 0, 0)
    calls = [
        ((2, None, C.byref(good), _p(hits), _p(back)), ARG), ((2, _p(pos), None, _p(hits), _p(back)), ARG),
        ((2, _p(pos), C.byref(good), None, _p(back)), ARG), ((2, _p(pos), C.byref(good), _p(hits), None), ARG),
        ((2, _p(pos), C.byref(api.ProbeParams(0, 4, 0, 1)), _p(hits), _p(back)), ARG),
        ((2, _p(pos), C.byref(api.ProbeParams(0, 0, 0, 0)), _p(hits), _p(back)), ARG),
        ((2, _p(pos), C.byref(api.ProbeParams(0, 4, 0xFFFFFFFF, 0)), _p(hits), _p(back)), ARG),
        ((2, _p(pos), C.byref(api.ProbeParams(0xFFFFFFFF, 2, 0, 0)), _p(hits), _p(back)), ARG),
    ]
    for args, code in calls:
        assert L.pt_probe_backfaces(r.ctx, *args) == code, code
    bad = pos.copy(); bad[1, 2] = np.nan
    assert L.pt_probe_backfaces(r.ctx, 2, _p(bad), C.byref(good), _p(hits), _p(back)) == ARG
    assert L.pt_probe_backfaces(r.ctx, 0, None, None, None, None) == 0
    sh = np.zeros(54, F)
    for args, code in calls[:2] + calls[4:]:                                        # the bake refuses the same calls
        assert L.pt_bake_probes(r.ctx, args[0], args[1], args[2], _p(sh)) == code


@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("bias", [0.0, 0.375])
def test_host_lookup_is_the_restatement(api, count, bias):
    r, _ = _renderer(api)
    g = PG.random_grid(count, 11 + sum(count), bias=bias)
    g.set_on(r)
    P, n = PG.query_points(g, 300, 12)
    want, want_lit = PG.lookup(g, P, n)
    got, lit = r.probe_grid_lookup(P, n)
    assert_bit_equal(got, want, f"{count}, bias {bias}")
    assert np.array_equal(lit, want_lit) and lit.all()
    if bias == 0.0:
        # the exact case: at a node's own position the result is max(e_node, 0) bit for bit, under any normal
        nodes = g.nodes().reshape(-1, 3)
        for normal in PG.unit_normals(3, 13):
            e = PG.node_evaluation(g, normal).reshape(-1, 3)
            got = r.probe_grid_lookup(nodes, np.repeat(normal[None], len(nodes), axis=0))[0]
            assert_bit_equal(got, np.where(e > 0, e, F(0.0)).astype(F), f"{count}: nodes")
    if count == (1, 1, 1):
        # one probe: its evaluation everywhere
        e = PG.node_evaluation(g, n[0]).reshape(3)
        got = r.probe_grid_lookup(P, np.repeat(n[:1], len(P), axis=0))[0]
        assert_bit_equal(got, np.repeat(np.where(e > 0, e, F(0.0)).astype(F)[None], len(P), axis=0), "1 x 1 x 1")


def test_a_swapped_index_order_would_show(api):
    """3 x 2 x 4: a grid whose coefficients depend on one index alone is flat along the other two axes"""
    r, _ = _renderer(api)
    for axis in range(3):
        g = PG.random_grid((3, 2, 4), 3)
        idx = np.arange(g.count[axis], dtype=F).reshape([-1 if a == 2 - axis else 1 for a in range(3)] + [1])
        g.sh = np.zeros_like(g.sh)
        g.sh[..., 0, :] = idx + F(1.0)
        g.set_on(r)
        P, n = PG.query_points(g, 200, 21 + axis)
        finite = np.isfinite(P).all(axis=1)
        got = r.probe_grid_lookup(P[finite], n[finite])[0]
        x = np.clip((P[finite, axis] - g.origin[axis]) / g.cell[axis], 0, g.count[axis] - 1)
        assert np.allclose(got[:, 0], (x + 1.0) * 0.2820948, rtol=1e-5), axis


def test_invalid_nodes_are_left_out_and_never_read(api):
    r, _ = _renderer(api)
    g = PG.random_grid((3, 2, 4), 17, invalid=0.35)
    assert 4 < g.valid.sum() < 20
    g.set_on(r)
    P, n = PG.query_points(g, 400, 18)
    want, want_lit = PG.lookup(g, P, n)
    got, lit = r.probe_grid_lookup(P, n)
    assert_bit_equal(got, want, "renormalised over the valid corners")
    assert np.array_equal(lit, want_lit) and lit.any()
    # an invalid node's coefficients never reach the result: change them and the bits stay
    other = PG.Grid(g.origin, g.cell, g.count, np.where(g.valid[..., None, None], g.sh, F(1e30)), g.valid, g.bias)
    other.set_on(r)
    again = r.probe_grid_lookup(P, n)
    assert_bit_equal(again[0], got, "invalid nodes' coefficients changed")
    assert np.array_equal(again[1], lit)
    assert r.probe_grid_info()[4] == int(g.valid.sum())
    # a cell with all eight corners invalid is not lit, and its neighbours still are
    valid = np.ones((4, 2, 3), bool)
    valid[0:2, :, 0:2] = False
    dark = PG.Grid(g.origin, g.cell, g.count, g.sh, valid)
    dark.set_on(r)
    inside = dark.origin + dark.cell * np.array([[0.5, 0.5, 0.5], [0.25, 0.75, 0.9], [0.0, 0.0, 0.0]], F)
    edge = dark.origin + dark.cell * np.array([[1.5, 0.5, 0.5], [0.5, 0.5, 1.5]], F)
    nn = PG.unit_normals(5, 19)
    got, lit = r.probe_grid_lookup(np.concatenate([inside, edge]), nn)
    assert lit.tolist() == [0, 0, 0, 1, 1] and not got[:3].any()
    want, want_lit = PG.lookup(dark, np.concatenate([inside, edge]), nn)
    assert_bit_equal(got, want, "dark cell")
    assert np.array_equal(lit, want_lit)


def test_negative_evaluations_are_clamped(api):
    r, _ = _renderer(api)
    sh = np.zeros((2, 2, 2, 9, 3), F)
    sh[..., 0, :] = F(-1.0)                                                        # a negative constant: every evaluation is negative
    sh[..., 0, 1] = F(2.0)
    g = PG.Grid((0, 0, 0), (1, 1, 1), (2, 2, 2), sh)
    g.set_on(r)
    P, n = PG.query_points(g, 50, 23)
    got, lit = r.probe_grid_lookup(P, n)
    assert lit.all() and (got[:, 0] == 0).all() and (got[:, 2] == 0).all() and (got[:, 1] > 0.5).all()
    assert not np.signbit(got).any()


def test_a_constant_radiance_comes_back_as_itself(api):
    """the unit convention: probes that hold the SH projection of the constant radiance c light any surface with c (irradiance over pi, the
    lightmap's unit); through the sums as well, where the factor 4 pi / n is the wrapper's"""
    r, _ = _renderer(api)
    c = np.array([0.75, 2.0, 0.125])
    sh = np.broadcast_to(PG.constant_radiance_sh(c), (4, 2, 3, 9, 3)).copy()
    g = PG.Grid((-1.0, 0.5, 2.0), (0.5, 2.0, 0.25), (3, 2, 4), sh)
    g.set_on(r)
    P, n = PG.query_points(g, 200, 29)
    got, lit = r.probe_grid_lookup(P, n)
    assert lit.all() and np.abs(got.astype(np.float64) / c - 1.0).max() < 1e-5
    # a bake of n_samples samples of constant radiance c has the sums c * y0 * n_samples in band 0
    n_samples = 48
    sums = np.zeros((4, 2, 3, 9, 3), np.float64)
    sums[..., 0, :] = c * 0.28209479177387814 * n_samples
    r.set_probe_grid_sums(g.origin, g.cell, sums.astype(F), n_samples)
    got, lit = r.probe_grid_lookup(P, n)
    assert lit.all() and np.abs(got.astype(np.float64) / c - 1.0).max() < 1e-5
    with pytest.raises(api.PtError):
        r.set_probe_grid_sums(g.origin, g.cell, sums.astype(F), 0)


def test_the_grid_is_world_space_data(api):
    """it survives pt_build, pt_set_instances, pt_set_model_uvs and pt_set_lightmap, and only the clearing call clears it"""
    r, sc = _renderer(api)
    _, model = LC.cornell_atlas_scene()
    g = PG.random_grid((3, 2, 4), 37, invalid=0.2)
    g.set_on(r)
    P, n = PG.query_points(g, 100, 38)
    before, info = r.probe_grid_lookup(P, n), r.probe_grid_info()

    def same(what):
        now = r.probe_grid_lookup(P, n)
        assert_bit_equal(now[0], before[0], what)
        assert np.array_equal(now[1], before[1]) and r.probe_grid_info()[2:] == info[2:], what
    r.rebuild(); same("pt_build")
    moved = np.array([[1, 0, 0, 0.5, 0, 1, 0, 0.25, 0, 0, 1, -0.5]], F).reshape(1, 3, 4)
    r.set_instances(model, moved); r.rebuild(); same("pt_set_instances")
    r.set_lightmap(model, 0, np.ones((2, 2, 3), F)); same("pt_set_lightmap")
    r.set_model_uvs(model, None); same("pt_set_model_uvs")
    r.set_probe_grid(None, None, None)
    assert r.probe_grid_info()[2] == (0, 0, 0)
    with pytest.raises(api.PtError):
        r.probe_grid_lookup(P, n)


def test_probe_grid_positions_are_origin_plus_index_times_cell(api):
    pos = api.Renderer.probe_grid_positions((-1.0, 0.5, 2.0), (0.5, 2.0, 0.25), (3, 2, 4))
    g = PG.random_grid((3, 2, 4), 1)
    assert pos.shape == (4, 2, 3, 3) and np.array_equal(pos, g.nodes())
    assert pos[3, 1, 2].tolist() == [0.0, 2.5, 2.75]
