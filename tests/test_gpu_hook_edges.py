"""GPU (-m gpu): the edges every staged entry of the C-ABI shares, whatever it computes.  No elements: PT_OK, empty outputs, and no launch
error left with the runtime for the next entry to report.  Block edges: one element, one short of the hooks' 256-thread block, a block, one
over, against the hook's host twin or the oracle, compared exactly as the hook's own test compares (cited at each).  Optional outputs and
inputs: the result does not depend on what the caller declined.  pt_last_batch_shade_pids waits for the batch it reads."""
import ctypes as C

import numpy as np
import pytest

import baked_common as BC
import lightmap_denoise_common as LD
import normalmap_common as NM
import probe_grid_common as PG
import probe_radiance_common as PR
from conftest import assert_bit_equal
from temporal_common import random_case

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
SIZES = (1, 255, 256, 257)          # around the hooks' 256-thread blocks
N = SIZES[-1]
Q_LAMBERT = 1                       # pt_types.h: the Lambertian shade queue


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_S = {}


def shared(api):
    """the scenes, renderers and queries of this file: made once and left unchanged"""
    if _S:
        return _S
    from path_tracer_amd import scenes
    _S["mixed"] = scenes.cornell_mixed(64, 64)
    _S["r"] = api.Renderer(_S["mixed"], 64, 64, max_bounces=4)           # the one Renderer of the empty calls
    grid = PG.random_grid((3, 2, 4), 50, invalid=0.3, bias=0.375)
    grid.set_on(_S["r"])
    P, n, d, a = PR.query(grid, N, 42)
    _S["grid"], _S["points"] = grid, (P[:N], n[:N], d[:N], a[:N])
    PR.random_radiance(grid, 4, (0.35,), 47).set_on(_S["r"])
    _S["nm_desc"] = NM.hook_scene()
    _S["nm"] = api.Renderer(_S["nm_desc"], 16, 16)
    _S["nm_q"] = NM.hook_queries(_S["nm_desc"], N)
    soup, maps = BC.soup_scene()
    _S["soup"] = api.Renderer(soup, 48, 32)
    BC.set_maps(_S["soup"], maps)
    _S["soup_q"] = BC.soup_queries(soup, N)
    rng = np.random.default_rng(5)
    O = rng.uniform(-270, 270, (N, 3)).astype(F)
    O[:, 1] += 50
    D = rng.normal(size=(N, 3))
    _S["rays"] = (O, (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F), rng.uniform(0, 800, N).astype(F))
    nrm = rng.normal(size=(N, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    inc = rng.normal(size=(N, 3)); inc = (inc / np.linalg.norm(inc, axis=1, keepdims=True)).astype(F)
    flip = (inc * nrm).sum(1) > 0
    inc[flip] = -inc[flip]
    out = rng.normal(size=(N, 3)); out = (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(F)
    _S["surface"] = (inc, nrm, (np.arange(N) % 2).astype(np.uint8), rng.integers(0, 1 << 20, N).astype(U), rng.integers(0, 256, N).astype(U), out)
    return _S


# ---------------------------------------------------------------------------------------------------------------------------- no elements
Z3, Z1, ZU, ZB = np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, U), np.zeros(0, np.uint8)

EMPTY = [
    ("surface_colour host", lambda r: r.surface_colour(ZU, ZU, Z1, Z1)),
    ("surface_colour", lambda r: r.surface_colour(ZU, ZU, Z1, Z1, on_device=True)),
    ("shading_normal host", lambda r: r.shading_normal(ZU, ZU, Z1, Z1, Z3)),
    ("shading_normal", lambda r: r.shading_normal(ZU, ZU, Z1, Z1, Z3, on_device=True)),
    ("lightmap_lookup host", lambda r: r.lightmap_lookup(ZU, ZU, Z1, Z1)),
    ("lightmap_lookup", lambda r: r.lightmap_lookup(ZU, ZU, Z1, Z1, on_device=True)),
    ("lightmap_lookup_directional host", lambda r: r.lightmap_lookup_directional(ZU, ZU, Z1, Z1, Z3)),
    ("lightmap_lookup_directional", lambda r: r.lightmap_lookup_directional(ZU, ZU, Z1, Z1, Z3, on_device=True)),
    ("probe_grid_lookup host", lambda r: r.probe_grid_lookup(Z3, Z3)),
    ("probe_grid_lookup", lambda r: r.probe_grid_lookup(Z3, Z3, on_device=True)),
    ("probe_grid_specular host", lambda r: r.probe_grid_specular(Z3, Z3, Z3, Z1)),
    ("probe_grid_specular", lambda r: r.probe_grid_specular(Z3, Z3, Z3, Z1, on_device=True)),
    ("guide_follow_dir host", lambda r: r.guide_follow_dir(0, Z3, Z3, ZB)),
    ("guide_follow_dir", lambda r: r.guide_follow_dir(0, Z3, Z3, ZB, on_device=True)),
    ("trace_closest", lambda r: tuple(r.trace_closest(Z3, Z3).values())),
    ("trace_closest tmax", lambda r: tuple(r.trace_closest(Z3, Z3, Z1, which=1).values())),
    ("trace_any", lambda r: r.trace_any(Z3, Z3, Z1)),
    ("ss_sobol", lambda r: r.ss_sobol(512, ZU, ZU)),
    ("math_batch", lambda r: r.math_batch(0, Z1)),
    ("math_batch b", lambda r: r.math_batch(3, Z1, Z1)),
    ("material_eval", lambda r: r.material_eval(0, Z3, Z3, ZB, ZU, ZU, 1)),
    ("volume_eval", lambda r: r.volume_eval(0, Z3, Z1, Z1, ZU, ZU, 1)),
    ("bsdf_eval", lambda r: r.bsdf_eval(0, Z3, Z3, Z3, ZB)),
    ("integrate_rays", lambda r: r.integrate_rays(Z3, Z3, ZU, ZU)),
    ("bake_probes", lambda r: r.bake_probes(Z3, 4)),
    ("probe_backfaces", lambda r: r.probe_backfaces(Z3, 4)),
    ("bake_probe_depth", lambda r: r.bake_probe_depth(Z3, 4, 4, 10.0)),
    ("bake_probe_radiance", lambda r: r.bake_probe_radiance(Z3, 4, 4)),
    ("probe_radiance_prefilter host", lambda r: r.probe_radiance_prefilter(np.zeros((0, 16, 3), F), np.zeros((0, 16), U), (0.35,), on_device=False)),
    ("probe_radiance_prefilter", lambda r: r.probe_radiance_prefilter(np.zeros((0, 16, 3), F), np.zeros((0, 16), U), (0.35,))),
    ("last_batch_shade_pids", lambda r: (r.render_device(0, 1), r.last_batch_shade_pids(Q_LAMBERT, 0, 0))[1]),
]


@pytest.mark.parametrize("name, call", EMPTY, ids=[e[0] for e in EMPTY])
def test_no_elements_is_ok_and_leaves_no_error_behind(api, name, call):
    r = shared(api)["r"]
    out = call(r)                                                        # (a failure raises PtError)
    for a in out if isinstance(out, tuple) else (out,):
        assert a.size == 0, name
    # ... and the next entry that asks the runtime for its launch error finds none
    one = r.surface_colour(np.zeros(1, U), np.zeros(1, U), np.full(1, 0.25, F), np.full(1, 0.25, F), on_device=True)
    assert_bit_equal(one, r.surface_colour(np.zeros(1, U), np.zeros(1, U), np.full(1, 0.25, F), np.full(1, 0.25, F)), f"after an empty {name}")


# ---------------------------------------------------------------------------------------------------------------------------- block edges
@pytest.mark.parametrize("n", SIZES)
def test_host_twins_at_block_edges(api, n):
    s = shared(api)
    inst, prim, u, v, d = (a[:n] for a in s["nm_q"])
    # bit for bit, as test_gpu_textures.py::test_surface_colour_on_the_device_is_the_host_evaluation
    assert_bit_equal(s["nm"].surface_colour(inst, prim, u, v, on_device=True), s["nm"].surface_colour(inst, prim, u, v), f"surface colour, {n}")
    # bit for bit and equal flags, as test_gpu_normalmap.py::test_shading_normal_on_the_device_is_the_host_evaluation
    host, hfront = s["nm"].shading_normal(inst, prim, u, v, d)
    dev, dfront = s["nm"].shading_normal(inst, prim, u, v, d, on_device=True)
    assert_bit_equal(dev, host, f"shading normal, {n}"); assert np.array_equal(dfront, hfront)
    # bit for bit and equal flags, as test_gpu_probe_grid.py::test_device_lookup_is_the_host_lookup
    P, nn, dd, a = (x[:n] for x in s["points"])
    host, dev = s["r"].probe_grid_lookup(P, nn), s["r"].probe_grid_lookup(P, nn, on_device=True)
    assert_bit_equal(dev[0], host[0], f"probe grid lookup, {n}"); assert np.array_equal(dev[1], host[1])
    # bit for bit and equal flags, as test_gpu_probe_radiance.py::test_device_specular_lookup_is_the_host_lookup
    host, dev = s["r"].probe_grid_specular(P, nn, dd, a), s["r"].probe_grid_specular(P, nn, dd, a, on_device=True)
    assert_bit_equal(dev[0], host[0], f"probe grid specular, {n}"); assert np.array_equal(dev[1], host[1])
    # bit for bit, every material, as test_gpu_guides_follow.py::test_unit_hook_on_the_device_is_the_host_evaluation
    inc, nrm, front = (x[:n] for x in s["surface"][:3])
    for mi in range(len(s["mixed"].materials())):
        assert_bit_equal(s["r"].guide_follow_dir(mi, inc, nrm, front, on_device=True), s["r"].guide_follow_dir(mi, inc, nrm, front), f"follow dir, material {mi}, {n}")
    # bit for bit and equal flags, as test_gpu_baked.py::test_device_lookup_is_the_host_lookup
    q = tuple(x[:n] for x in s["soup_q"])
    host, dev = s["soup"].lightmap_lookup(*q), s["soup"].lightmap_lookup(*q, on_device=True)
    assert_bit_equal(dev[0], host[0], f"lightmap lookup, {n}"); assert np.array_equal(dev[1], host[1])


def oracle_twins(api, O):
    """the oracle's answers for all N rows of every hook below: computed once"""
    s = shared(api)
    if "want" not in s:
        from path_tracer_amd.scene_desc import Volume
        from test_oracle_kat import volume_eval_inputs, volume_probe_scene
        orc = O.Oracle(s["mixed"])
        inc, nrm, front, px, sm, out = s["surface"]
        ro, rd, tm = s["rays"]
        from path_tracer_amd.scene_desc import EMISSIVE
        w = {"materials": [mi for mi, m in enumerate(s["mixed"].materials()) if m.kind != EMISSIVE]}      # Lambertian, GGX metal, dielectric
        w["material"] = {mi: np.stack([orc.material_eval(mi, inc[i], nrm[i], front[i], int(px[i]), int(sm[i]), 3) for i in range(N)]) for mi in w["materials"]}
        w["bsdf"] = {mi: orc.bsdf_eval(mi, inc, out, nrm, front) for mi in w["materials"]}
        w["sobol"] = np.stack([O.ss_sobol(100000, int(i), int(k)) for i, k in zip(px, sm)])
        w["closest"] = [orc.trace_closest(ro, rd, None, which) for which in (0, 1)]
        w["any"] = [orc.trace_any(ro, rd, tm, which) for which in (0, 1)]
        vsc = volume_probe_scene(Volume.new((0.4, 0.0, 0.9), 0.05, 1.0 / 50.0, 0.3))
        s["vol_r"], s["vol_mi"], s["vol_in"] = api.Renderer(vsc, 8, 8), len(vsc.materials()) - 1, volume_eval_inputs(N, 11)
        vo = O.Oracle(vsc)
        vi, vt, vd, vp, vs = s["vol_in"]
        w["volume"] = np.stack([vo.volume_eval(s["vol_mi"], vi[i], vt[i], vd[i], int(vp[i]), int(vs[i]), 2) for i in range(N)])
        s["want"] = w
    return s, s["want"]


@pytest.mark.parametrize("n", SIZES)
def test_oracle_twins_at_block_edges(api, oracle_mod, n):
    s, w = oracle_twins(api, oracle_mod)
    r = s["r"]
    inc, nrm, front, px, sm, out = (x[:n] for x in s["surface"])
    for mi in w["materials"]:
        # bit for bit, as test_gpu_parity.py::test_materials_match_oracle and test_gpu_materials.py's first-n-rows loops
        assert_bit_equal(r.material_eval(mi, inc, nrm, front, px, sm, 3), w["material"][mi][:n], f"material_eval {mi}, {n}")
        assert_bit_equal(r.bsdf_eval(mi, inc, out, nrm, front), w["bsdf"][mi][:n], f"bsdf_eval {mi}, {n}")
    # bit for bit, as test_gpu_media.py::test_volume_eval_matches_oracle_and_binary64
    assert_bit_equal(s["vol_r"].volume_eval(s["vol_mi"], *(x[:n] for x in s["vol_in"]), 2), w["volume"][:n], f"volume_eval, {n}")
    # bit for bit, as test_gpu_parity.py::test_device_sobol_matches_known_answers
    assert_bit_equal(r.ss_sobol(100000, px, sm), w["sobol"][:n], f"ss_sobol, {n}")
    # every field bit for bit and equal hit flags, as test_gpu_parity.py::test_trace_matches_oracle_on_random_rays
    ro, rd, tm = (x[:n] for x in s["rays"])
    for which in (0, 1):
        g = r.trace_closest(ro, rd, None, which)
        for k in ("inst", "prim", "t", "u", "v"):
            assert_bit_equal(g[k], w["closest"][which][k][:n], f"tlas{which} closest.{k}, {n}")
        assert np.array_equal(r.trace_any(ro, rd, tm, which), w["any"][which][:n]), f"tlas{which} any, {n}"


# ------------------------------------------------------------------------------------------------------------------------ optional arrays
def test_lightmap_denoise_with_and_without_the_area(api):
    sc, model = LD.scene("box")
    r = api.Renderer(sc, 16, 16)
    sums, sumsq = LD.synthetic(37, 19, LD.N_SAMPLES, seed=3)
    for sq in (sumsq, None):
        both = r.denoise_lightmap(model, 0, sums, LD.N_SAMPLES, sumsq=sq, on_device=True, want_area=True)
        alone = r.denoise_lightmap(model, 0, sums, LD.N_SAMPLES, sumsq=sq, on_device=True)
        assert_bit_equal(alone, both[0], "the filtered map does not depend on whether the area is asked for")
        assert (both[1] > 0).any()


def test_math_batch_without_b_and_without_o1(api):
    r = shared(api)["r"]
    a = np.random.default_rng(9).uniform(0, 6, N).astype(F)
    zeros = np.zeros(N, F)
    s, c = r.math_batch(0, a, zeros)                                     # sin | cos with every array there
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    o0, o1 = np.zeros(N, F), np.zeros(N, F)
    assert r.L.pt_math_batch(r.ctx, 0, N, p(a), None, p(o0), p(o1)) == 0
    assert_bit_equal(o0, s, "b NULL reads as zeros: o0"); assert_bit_equal(o1, c, "b NULL reads as zeros: o1")
    o0[:] = 0
    assert r.L.pt_math_batch(r.ctx, 0, N, p(a), p(zeros), p(o0), None) == 0
    assert_bit_equal(o0, s, "o1 NULL: o0 is what it was")
    o0[:] = 0
    assert r.L.pt_math_batch(r.ctx, 0, N, p(a), None, p(o0), None) == 0
    assert_bit_equal(o0, s, "b and o1 NULL")


def test_post_temporal_with_and_without_its_optional_images(api):
    r = shared(api)["r"]
    w, h = 37, 19
    prev, cur, xprev, nprev, vel = random_case(np.random.default_rng(77), w, h)
    names = ("history", "moments", "variance")
    forms = dict(none={}, all=dict(xprev=xprev, nprev=nprev, velocity=vel), velocity=dict(velocity=vel), rest=dict(xprev=xprev, nprev=nprev))
    got = {}
    for form, kw in forms.items():
        # device against host bit for bit, as test_gpu_temporal.py::test_device_path_equals_the_host_path_and_the_restatement
        got[form] = r.post_temporal(prev, cur, on_device=True, **kw)
        for d, hs, name in zip(got[form], r.post_temporal(prev, cur, on_device=False, **kw), names):
            assert_bit_equal(d, hs, f"{form}: {name}")
    # what a NULL stands for, handed over: xprev NULL is the position, nprev NULL the normal
    for d, e, name in zip(r.post_temporal(prev, cur, on_device=True, xprev=cur[1], nprev=cur[2]), got["none"], names):
        assert_bit_equal(d, e, f"the defaults spelled out: {name}")
    for d, e, name in zip(r.post_temporal(prev, cur, on_device=True, xprev=cur[1], nprev=cur[2], velocity=vel), got["velocity"], names):
        assert_bit_equal(d, e, f"the defaults spelled out beside a velocity: {name}")


# ------------------------------------------------------------------------------------------------------------------ the shade queue's ids
def test_shade_pids_wait_for_the_batch(api, cornell64):
    r = api.Renderer(cornell64, 64, 64, max_bounces=4)
    count = 2048
    r.render_device(0, 2)
    early = r.last_batch_shade_pids(Q_LAMBERT, 0, count)                 # straight after the launches: the call itself waits
    r.synchronize()
    late = r.last_batch_shade_pids(Q_LAMBERT, 0, count)
    assert early.shape == (count,) and np.array_equal(early, late)
    assert len(np.unique(late)) > 1, "path ids, not a constant"
    out = np.zeros(1, U)
    assert r.L.pt_last_batch_shade_pids(r.ctx, Q_LAMBERT, 0, 0, out.ctypes.data_as(C.c_void_p)) == 0
    assert r.L.pt_last_batch_shade_pids(r.ctx, Q_LAMBERT, 0, 0, None) == 0
    r.close()
