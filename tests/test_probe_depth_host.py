"""CPU: probe visibility (pt_probe_depth_texel, pt_bake_probe_depth, pt_set_probe_grid_depth, pt_get_probe_grid_depth_info) without a GPU: the
symbols, every refusal include/pt_api.h promises before any device call and their order, each with "nothing changed" checked, the octahedral
texel and the host lookup with visibility against the numpy restatement of tests/probe_depth_common.py bit for bit, the exact cases,
occlusion, the lifetime of depth, and the light leak of scenes.two_rooms measured from oracle pieces alone.  No GPU is touched (the bake, the
device lookup and the view: tests/test_gpu_probe_depth.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import lightmap_common as LC
import probe_depth_common as PD
import probe_grid_common as PG
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, STATE, LIMIT = -1, -3, -5
NEW_SYMBOLS = ["pt_bake_probe_depth", "pt_set_probe_grid_depth", "pt_get_probe_grid_depth_info"]


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


def _depth_struct(api, res=4, flags=0, vis_floor=0.0, reserved=(0, 0, 0, 0, 0)):
    return api.ProbeDepth(res, flags, vis_floor, (C.c_uint32 * 5)(*reserved))


# ---------------------------------------------------------------------------------------------------------------- exports and refusals
def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert "pt_probe_depth_texel" in api.EXPORTS and "int pt_probe_depth_texel(uint32_t res" in header
    assert "typedef struct pt_probe_depth_params" in header and C.sizeof(api.ProbeDepthParams) == 32
    assert "typedef struct pt_probe_depth" in header and C.sizeof(api.ProbeDepth) == 32 and api.PROBE_VIS_FACING == 1
    methods = ("bake_probe_depth", "set_probe_grid_depth", "set_probe_grid_depth_sums", "probe_grid_depth_info", "probe_depth_texel")
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for method in methods:
        assert callable(getattr(api.Renderer, method))
        assert method + "(" in wrapper, method
    assert "visibility or depth moments" not in header


def test_depth_refusals_and_their_order_change_nothing(api):
    r, _ = _renderer(api)
    L = r.L
    assert L.pt_set_probe_grid_depth(r.ctx, C.byref(_depth_struct(api)), _p(np.ones(8 * 16 * 2, F))) == STATE          # no grid yet
    assert L.pt_set_probe_grid_depth(r.ctx, C.byref(_depth_struct(api, res=0)), None) == STATE                            # not even to clear
    assert L.pt_set_probe_grid_depth(r.ctx, C.byref(_depth_struct(api, reserved=(0, 0, 0, 0, 1))), None) == ARG          # reserved before the grid
    g = PG.random_grid((3, 2, 4), 5, invalid=0.2, bias=0.25)
    g.set_on(r)
    depth = PD.random_depth(g, 4, 6, vis_floor=0.05, facing=True)
    depth.set_on(r)
    P, n = PG.query_points(g, 64, 6)
    before, info, dinfo, scene = r.probe_grid_lookup(P, n), r.probe_grid_info(), r.probe_grid_depth_info(), r.scene_info().as_dict()
    assert dinfo[0] == 4 and dinfo[1] == 1 and F(dinfo[2]) == F(0.05)
    assert_bit_equal(before[0], PD.lookup(g, depth, P, n)[0], "the depth that is set")
    good = np.ones((24, 16, 2), F)
    one = np.zeros(2, F)                 # never read past the checks: each of these is refused before a moment is

    def bad(value, which=1):
        a = good.copy()
        a[17, 9, which] = value
        return a
    nan, inf = float("nan"), float("inf")
    refusals = [
        (None, good, ARG),
        (dict(reserved=(1, 0, 0, 0, 0)), good, ARG), (dict(reserved=(0, 0, 0, 0, 7)), good, ARG),
        (dict(res=4), None, ARG), (dict(res=0), good, ARG),
        (dict(res=1), one, LIMIT), (dict(res=17), one, LIMIT), (dict(res=0xFFFFFFFF), one, LIMIT),
        (dict(flags=2), good, ARG), (dict(flags=3), good, ARG), (dict(flags=0x80000000), good, ARG),
        (dict(vis_floor=-0.25), good, ARG), (dict(vis_floor=1.5), good, ARG), (dict(vis_floor=nan), good, ARG), (dict(vis_floor=inf), good, ARG),
        (dict(), bad(nan), ARG), (dict(), bad(inf, 0), ARG), (dict(), bad(-1.0), ARG), (dict(), bad(-inf, 0), ARG),
        # where several apply: v, the reserved words, the pointer against res, the limit, the flags, the floor, the moments last
        (dict(reserved=(0, 1, 0, 0, 0), res=17), one, ARG), (dict(res=17, flags=2), one, LIMIT), (dict(res=1, vis_floor=nan), one, LIMIT),
        (dict(flags=2, vis_floor=2.0), one, ARG), (dict(vis_floor=2.0), bad(nan), ARG), (dict(res=0, flags=2), one, ARG),
    ]
    for kw, moments, code in refusals:
        vs = None if kw is None else C.byref(_depth_struct(api, **kw))
        assert L.pt_set_probe_grid_depth(r.ctx, vs, _p(moments)) == code, (kw, code)
        now = r.probe_grid_info()
        assert now[2:] == info[2:] and np.array_equal(now[0], info[0]) and r.probe_grid_depth_info() == dinfo and r.scene_info().as_dict() == scene
        after = r.probe_grid_lookup(P, n)
        assert_bit_equal(after[0], before[0], f"lookup after the refused call {kw}")
        assert np.array_equal(after[1], before[1])
    # a zero moment and vis_floor's two ends are legal
    zero = good.copy(); zero[3, 2] = 0.0
    for floor in (0.0, 1.0):
        assert L.pt_set_probe_grid_depth(r.ctx, C.byref(_depth_struct(api, vis_floor=floor)), _p(zero)) == 0
    assert r.probe_grid_depth_info() == (4, 0, 1.0) and r.scene_info().as_dict() == scene and r.probe_grid_info()[2:] == info[2:]
    assert L.pt_get_probe_grid_depth_info(r.ctx, None) == 0 and L.pt_get_probe_grid_depth_info(None, None) == ARG


def test_bake_refusals_are_the_census_refusals_and_three_more(api):
    r, _ = _renderer(api)
    L = r.L
    pos = np.zeros((2, 3), F); sums = np.zeros((2, 16, 2), F); counts = np.zeros((2, 16), np.uint32)

    def prm(first=0, n=4, key=0, res=4, far=10.0, reserved=(0, 0, 0)):
        return C.byref(api.ProbeDepthParams(first, n, key, res, far, (C.c_uint32 * 3)(*reserved)))
    nan, inf = float("nan"), float("inf")
    calls = [
        ((2, None, prm(), _p(sums), _p(counts)), ARG), ((2, _p(pos), None, _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(), None, _p(counts)), ARG), ((2, _p(pos), prm(), _p(sums), None), ARG),
        ((2, _p(pos), prm(n=0), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(key=0xFFFFFFFF), _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(first=0xFFFFFFFF, n=2), _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(res=1), _p(sums), _p(counts)), LIMIT), ((2, _p(pos), prm(res=17), _p(sums), _p(counts)), LIMIT),
        ((2, _p(pos), prm(res=0), _p(sums), _p(counts)), LIMIT),
        ((2, _p(pos), prm(far=0.0), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(far=-1.0), _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(far=nan), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(far=inf), _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(reserved=(1, 0, 0)), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(reserved=(0, 0, 9)), _p(sums), _p(counts)), ARG),
        # the order: the census' own, then res, max_distance, the reserved words
        ((2, _p(pos), prm(n=0, res=17), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(res=17, far=nan), _p(sums), _p(counts)), LIMIT),
        ((2, _p(pos), prm(res=17, reserved=(1, 0, 0)), _p(sums), _p(counts)), LIMIT),
    ]
    for args, code in calls:
        assert L.pt_bake_probe_depth(r.ctx, *args) == code, code
    bad = pos.copy(); bad[1, 2] = np.nan
    assert L.pt_bake_probe_depth(r.ctx, 2, _p(bad), prm(), _p(sums), _p(counts)) == ARG
    assert L.pt_bake_probe_depth(r.ctx, 2, _p(bad), prm(res=17), _p(sums), _p(counts)) == ARG                 # the position before res
    assert L.pt_bake_probe_depth(r.ctx, 0, None, None, None, None) == 0
    assert not sums.any() and not counts.any()
    # the texel hook
    d = np.ones((3, 3), F); out = np.zeros(3, np.uint32)
    for res in (0, 1, 17):
        assert L.pt_probe_depth_texel(res, 3, _p(d), _p(out)) == LIMIT
    assert L.pt_probe_depth_texel(4, 3, None, _p(out)) == ARG and L.pt_probe_depth_texel(4, 3, _p(d), None) == ARG
    assert L.pt_probe_depth_texel(4, 0, None, None) == 0


# -------------------------------------------------------------------------------------------------------------------------- the texel
def _texel_inputs():
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    diagonals = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    phi = np.linspace(0.0, 2.0 * np.pi, 97)
    equator = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], axis=1)
    below = equator.copy(); below[:, 2] = -0.0
    # the fold lines |px| + |py| = 1 are the equator's image; approach them from both hemispheres as well
    near = np.concatenate([equator + [0, 0, 1e-7], equator - [0, 0, 1e-7]])
    odd = np.array([[0, 0, 0], [-0.0, 0.0, -0.0], [np.nan, 1, 0], [1, np.nan, 0], [1, 0, np.nan], [np.inf, 1, 0], [1, -np.inf, 0], [0, 1, np.inf],
                    [0, 1, -np.inf], [np.inf, np.inf, np.inf], [1e30, -1e30, 1e30], [3e38, 3e38, -3e38], [1e-40, 1e-42, -1e-41]])
    rnd = np.random.default_rng(71).normal(size=(4096, 3))
    return np.concatenate([axes, diagonals, equator, below, near, odd, rnd]).astype(F)


@pytest.mark.parametrize("R", [2, 3, 8, 16])
def test_texel_is_the_restatement(api, R):
    r, _ = _renderer(api)
    v = _texel_inputs()
    got = r.probe_depth_texel(v, R)
    assert np.array_equal(got, PD.oct_texel(v, R)) and got.max() < R * R
    zero = np.zeros((1, 3), F)
    assert r.probe_depth_texel(zero, R)[0] == 0                                     # a NaN lands on texel 0
    # the equator with +0.0 and -0.0 is one set of texels: -0.0 is not below
    phi = np.linspace(0.0, 2.0 * np.pi, 97)
    eq = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], axis=1).astype(F)
    neg = eq.copy(); neg[:, 2] = F(-0.0)
    assert np.signbit(neg[:, 2]).all() and np.array_equal(r.probe_depth_texel(eq, R), r.probe_depth_texel(neg, R))
    # each texel's centre direction maps back to it, so every texel is hit (R = 3 and 4 below as well)
    centres = PD.oct_centre_directions(R)
    assert np.array_equal(r.probe_depth_texel(centres, R), np.arange(R * R))
    # the map is scale-free
    rnd = v[-4096:]
    base = r.probe_depth_texel(rnd, R)
    for scale in (1e-20, 1e20):
        scaled = (rnd * F(scale)).astype(F)
        assert np.array_equal(r.probe_depth_texel(scaled, R), PD.oct_texel(scaled, R))
        assert np.array_equal(r.probe_depth_texel(scaled, R), base), scale


@pytest.mark.parametrize("R", [3, 4])
def test_random_directions_hit_every_texel(api, R):
    r, _ = _renderer(api)
    got = r.probe_depth_texel(np.random.default_rng(72).normal(size=(4096, 3)).astype(F), R)
    assert np.array_equal(np.unique(got), np.arange(R * R))
    assert np.bincount(got, minlength=R * R).min() > 4096 // (R * R) // 4              # and none is starved: the map is near equal-area


# ------------------------------------------------------------------------------------------------------------------------- the lookup
@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("R", [2, 4, 8])
def test_host_lookup_with_depth_is_the_restatement(api, count, R):
    r, _ = _renderer(api)
    checked = 0
    for bias, invalid in ((0.0, 0.0), (0.375, 0.25)):
        g = PG.random_grid(count, 11 + sum(count), invalid=invalid, bias=bias)
        g.set_on(r)
        P, n = PG.query_points(g, 300, 12)
        plain = PG.lookup(g, P, n)[0]
        for facing in (False, True):
            for floor in (0.0, 0.05):
                for consistent in (True, False):
                    depth = PD.random_depth(g, R, 13 + R, floor, facing, consistent)
                    depth.set_on(r)
                    want, want_lit = PD.lookup(g, depth, P, n)
                    got, lit = r.probe_grid_lookup(P, n)
                    assert_bit_equal(got, want, f"{count}, R {R}, bias {bias}, facing {facing}, floor {floor}, consistent {consistent}")
                    assert np.array_equal(lit, want_lit)
                    assert not np.array_equal(got, plain)                            # visibility changed something
                    checked += 1
    assert checked == 16


@pytest.mark.parametrize("count", PG.COUNTS)
def test_the_two_exact_cases(api, count):
    r, _ = _renderer(api)
    for bias in (0.0, 0.375):
        g = PG.random_grid(count, 21 + sum(count), invalid=0.2 if count != (1, 1, 1) else 0.0, bias=bias)
        g.set_on(r)
        P, n = PG.query_points(g, 300, 22)
        # far moments, FACING off: vis = 1 at every point whose distance to the nodes is a finite number below m1, and the result is the
        # plain lookup bit for bit.  (query_points' last eight rows are NaN, 1e30 and infinite: from there r is NaN or +inf, beyond any
        # finite m1; the restatement holds them, above.)
        reach = np.isfinite(P).all(axis=1) & (np.abs(P) < 1e20).all(axis=1)
        assert reach.sum() == P.shape[0] - 8
        plain, plain_lit = r.probe_grid_lookup(P, n)
        for R in (2, 8):
            PD.far_depth(g, R).set_on(r)
            got, lit = r.probe_grid_lookup(P, n)
            assert_bit_equal(got[reach], plain[reach], f"{count}, R {R}: far moments")
            assert np.array_equal(lit[reach], plain_lit[reach])
            assert_bit_equal(got[reach], PG.lookup(g, P[reach], n[reach])[0], "the plain restatement")
    # at a valid node's own position (bias 0: r = 0) the result is still max(e_node, 0), whatever the moments and the flags
    g = PG.random_grid(count, 23 + sum(count))
    g.set_on(r)
    nodes = g.nodes().reshape(-1, 3)
    for facing in (False, True):
        PD.random_depth(g, 4, 24, 0.0, facing).set_on(r)
        for normal in PG.unit_normals(3, 25):
            e = PG.node_evaluation(g, normal).reshape(-1, 3)
            got = r.probe_grid_lookup(nodes, np.repeat(normal[None], len(nodes), axis=0))[0]
            assert_bit_equal(got, np.where(e > 0, e, F(0.0)).astype(F), f"{count}: nodes, facing {facing}")


def test_occlusion(api):
    r, _ = _renderer(api)
    rng = np.random.default_rng(31)
    sh = rng.uniform(0.5, 2.0, (1, 1, 2, 9, 3)).astype(F)
    sh[..., 1:, :] *= F(0.1)
    g = PG.Grid((0.0, 0.0, 0.0), (4.0, 1.0, 1.0), (2, 1, 1), sh)
    g.set_on(r)
    R = 4
    # zero-variance moments: node 0 sees a wall at distance 1 in every direction, node 1 sees nothing nearer than 100
    wall = np.zeros((2, R * R, 2), F)
    wall[0] = (1.0, 1.0)
    wall[1] = (100.0, 10000.0)
    P = np.array([[3.0, 0.25, 0.5], [2.0, 0.0, 0.0], [1.5, 0.5, 0.5], [0.5, 0.0, 0.0]], F)       # the last one is on node 0's side of the wall
    n = PG.unit_normals(4, 32)
    PD.Depth(wall).set_on(r)
    got, lit = r.probe_grid_lookup(P, n)
    assert_bit_equal(got, PD.lookup(g, PD.Depth(wall), P, n)[0], "a wall before node 0")
    assert lit.all()
    # node 0 weighs exactly 0 beyond its wall: whatever it holds, the bits stay; on its own side it counts
    loud = g.sh.copy(); loud[0, 0, 0] = F(1e30)
    PG.Grid(g.origin, g.cell, g.count, loud).set_on(r)
    PD.Depth(wall).set_on(r)                                                       # (a new grid dropped the depth)
    again = r.probe_grid_lookup(P, n)[0]
    assert_bit_equal(again[:3], got[:3], "node 0 behind its wall")
    assert not np.array_equal(again[3], got[3])
    g.set_on(r)
    # every corner occluded: not lit with floor 0, lit with floor 0.05
    both = wall.copy(); both[1] = (0.5, 0.25)
    for floor, want_lit in ((0.0, 0), (0.05, 1)):
        d = PD.Depth(both, floor)
        d.set_on(r)
        got, lit = r.probe_grid_lookup(P[:3], n[:3])
        assert lit.tolist() == [want_lit] * 3
        assert_bit_equal(got, PD.lookup(g, d, P[:3], n[:3])[0], f"all occluded, floor {floor}")
        assert (got == 0).all() if not want_lit else (got > 0).any()


def test_invalid_nodes_moments_never_reach_the_result(api):
    r, _ = _renderer(api)
    g = PG.random_grid((3, 2, 4), 17, invalid=0.35)
    assert 4 < g.valid.sum() < 20
    g.set_on(r)
    P, n = PG.query_points(g, 400, 18)
    P, n = P[:-8], n[:-8]                                                          # (finite points: an infinite r makes NaN weights)
    depth = PD.random_depth(g, 4, 19, 0.05, True)
    depth.set_on(r)
    got, lit = r.probe_grid_lookup(P, n)
    assert_bit_equal(got, PD.lookup(g, depth, P, n)[0], "with invalid nodes")
    other = depth.moments.copy()
    other[~g.valid.reshape(-1)] = np.random.default_rng(20).uniform(0.0, 50.0, other[~g.valid.reshape(-1)].shape).astype(F)
    PD.Depth(other, 0.05, True).set_on(r)
    again = r.probe_grid_lookup(P, n)
    assert_bit_equal(again[0], got, "invalid nodes' moments changed")
    assert np.array_equal(again[1], lit)


# ------------------------------------------------------------------------------------------------------------------------ the lifetime
def test_depth_lives_with_its_grid(api):
    r, sc = _renderer(api)
    _, model = LC.cornell_atlas_scene()
    g = PG.random_grid((3, 2, 4), 37, invalid=0.2)
    g.set_on(r)
    assert r.probe_grid_depth_info() == (0, 0, 0.0)
    depth = PD.random_depth(g, 8, 38, 0.0, True)
    depth.set_on(r)
    P, n = PG.query_points(g, 100, 39)
    before = r.probe_grid_lookup(P, n)
    plain = PG.lookup(g, P, n)
    assert r.probe_grid_depth_info() == (8, 1, 0.0) and not np.array_equal(before[0], plain[0])

    def same(what):
        now = r.probe_grid_lookup(P, n)
        assert_bit_equal(now[0], before[0], what)
        assert np.array_equal(now[1], before[1]) and r.probe_grid_depth_info() == (8, 1, 0.0), what
    r.rebuild(); same("pt_build")
    moved = np.array([[1, 0, 0, 0.5, 0, 1, 0, 0.25, 0, 0, 1, -0.5]], F).reshape(1, 3, 4)
    r.set_instances(model, moved); r.rebuild(); same("pt_set_instances")
    r.set_lightmap(model, 0, np.ones((2, 2, 3), F)); same("pt_set_lightmap")
    # clearing depth: the plain lookup again, the grid still there; clearing what is not there is fine
    r.set_probe_grid_depth(None)
    assert r.probe_grid_depth_info() == (0, 0, 0.0) and r.probe_grid_info()[2] == (3, 2, 4)
    assert_bit_equal(r.probe_grid_lookup(P, n)[0], plain[0], "depth cleared")
    r.set_probe_grid_depth(None)
    # ANY pt_set_probe_grid drops depth: the same grid again, and the clearing call
    depth.set_on(r); same("set again")
    g.set_on(r)
    assert r.probe_grid_depth_info() == (0, 0, 0.0)
    assert_bit_equal(r.probe_grid_lookup(P, n)[0], plain[0], "the grid set again: depth dropped")
    depth.set_on(r)
    r.set_probe_grid(None, None, None)
    assert r.probe_grid_depth_info() == (0, 0, 0.0)
    with pytest.raises(api.PtError):
        depth.set_on(r)                                                            # no grid: nothing to set depth on
    # the wrapper's shape check and the sums' division
    g.set_on(r)
    with pytest.raises(api.PtError):
        r.set_probe_grid_depth(np.ones((23, 16, 2), F))
    sums = np.zeros((24, 4, 2), F); counts = np.zeros((24, 4), np.uint32)
    sums[:, 0] = (6.0, 14.0); counts[:, 0] = 3
    r.set_probe_grid_depth_sums(sums, counts, 5.0, 0.25)
    assert r.probe_grid_depth_info() == (2, 0, 0.25)
    m = PD.means(sums, counts, 5.0)
    assert m[0, 0].tolist() == [2.0, F(14.0) / F(3.0)] and m[0, 1].tolist() == [5.0, 25.0]
    assert np.array_equal(api.Renderer.probe_depth_means(sums, counts, 5.0), m)
    assert_bit_equal(r.probe_grid_lookup(P, n)[0], PD.lookup(g, PD.Depth(m, 0.25), P, n)[0], "through the sums")


# --------------------------------------------------------------------------------------------------------------------------- the leak
def test_depth_stops_the_leak_into_the_dark_room(api, oracle_mod):
    """scenes.two_rooms with a 4 x 2 x 2 grid, everything from the oracle: SH as probe_grid_common.oracle_probe_grid bakes it, depth from
    Oracle.trace_closest's t through the restated fold (R = 8, vis_floor 0).  The dark room's nodes hold exactly 0 and its true radiance is
    0; the plain lookup is > 0 at the points in the cells that straddle the partition (the leak), the lookup with depth is strictly smaller
    at every one of them.  No ratio is fixed in advance: the measured one is printed (profiles/r25_probe_depth.md)."""
    from path_tracer_amd import scenes
    sc = scenes.two_rooms(48, 32)
    orc = oracle_mod.Oracle(sc)
    r = api.Renderer(sc, 48, 32)
    grid, depth = PD.oracle_two_rooms(orc, r, sc)
    assert grid.count == (4, 2, 2) and grid.valid.all()
    x = grid.nodes()[0, 0, :, 0]
    assert x.tolist() == [-6.0, -2.0, 2.0, 6.0]                                    # the slab stands between node columns 1 and 2
    assert (grid.sh[:, :, 2:] == 0).all() and (grid.sh[:, :, :2, 0] > 0).all()     # the dark room's coefficients are exactly 0
    P, n, near = PD.dark_room_points()
    plain = BC_luminance(PG.lookup(grid, P, n)[0])
    seen = BC_luminance(PD.lookup(grid, depth, P, n)[0])
    assert (plain[:near] > 0).all(), plain[:near]                                  # the leak
    assert (seen[:near] < plain[:near]).all(), (seen[:near], plain[:near])
    assert (plain[near:] == 0).all() and (seen[near:] == 0).all()                  # beyond column 2 only dark nodes are blended
    ratio = float(seen[:near].mean() / plain[:near].mean())
    print(f"two_rooms, {near} points in the straddling cells: mean leaked luminance {plain[:near].mean():.5f} plain, {seen[:near].mean():.5f} with depth "
          f"(ratio {ratio:.4f}); worst point {float((seen[:near] / plain[:near]).max()):.4f}")
    # the truth is 0: nothing integrates to light in the sealed room
    rng = np.random.default_rng(81)
    for i in (0, 5, near - 1, near + 2):
        for s in range(8):
            d = PG._cosine_directions(n[i].astype(np.float64), 1, rng)[0].astype(F)
            start = (P[i] + F(1e-3) * n[i]).astype(F)
            assert not orc.integrate(start, d, i, s, 1, max_bounces=PD.TWO_ROOMS_BOUNCES)[0][:3].any()
    # the library's host lookup agrees with both
    grid.set_on(r)
    assert_bit_equal(r.probe_grid_lookup(P, n)[0], PG.lookup(grid, P, n)[0], "plain")
    depth.set_on(r)
    assert_bit_equal(r.probe_grid_lookup(P, n)[0], PD.lookup(grid, depth, P, n)[0], "with depth")


def BC_luminance(rgb):
    import baked_common as BC
    return BC.luminance(np.asarray(rgb, np.float64))
