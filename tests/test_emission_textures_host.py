"""CPU: emission textures (pt_set_material_emission_texture, include/pt_api.h) without a GPU — what the setter accepts and refuses, the light
sampler's weights against the numpy restatement and against the oracle's sampler of the equivalent untextured scene, what the setter costs a
build, the refusal of a sampler without weight, pt_surface_colour's host evaluation on lights, and the inputs of the GPU suite's plumbing test.
The renders are in tests/test_gpu_emission_textures.py."""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from emission_common import (F, N_LAMPS, dim_scene, emission_corner_scene, light_cdf, plumbing_prediction, plumbing_scene, scene_colour,
                             varying_light_scene, world_instance_models)

PT_ERR_ARG, PT_ERR_STATE = -1, -3
W, H, SPP = 32, 24, 2


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _two_lights():
    """varying_light_scene with a second, untextured light: the sampler mixes both kinds of weight"""
    from path_tracer_amd.scene_desc import Emissive, Model, SceneDesc
    from textures_common import quad
    desc = varying_light_scene(W, H)
    bp, bn = quad((6.0, 5.0, -1.0), (7.5, 5.0, -1.0), (7.5, 5.0, 2.0), (6.0, 5.0, 2.0))
    return SceneDesc.new(list(desc.models) + [Model.new(bp, bn, Emissive.new((2.0, 3.0, 1.0)), None, "bare")], desc.camera, desc.name)


def test_symbol_exported_and_bound(api):
    L = C.CDLL(api._build.LIB_PATH)
    name = "pt_set_material_emission_texture"
    assert name in api.EXPORTS and hasattr(L, name)
    assert getattr(api.lib(), name).argtypes is not None
    assert callable(api.Renderer.set_material_emission_texture)
    from path_tracer_amd.scene_desc import Emissive, Lambertian, Texture
    t = Texture.new(np.ones((1, 1, 3), F))
    assert Emissive.new((1, 1, 1)).emission_textured(t).emission_texture is t and Emissive.new((1, 1, 1)).emission_textured(t).texture is None
    with pytest.raises(AssertionError):
        Lambertian.new((1, 1, 1)).emission_textured(t)
    with pytest.raises(AssertionError):
        Emissive.new((1, 1, 1)).textured(t)                                      # Material.textured keeps its assert


def test_refusals_change_nothing(api):
    desc = _two_lights()
    r = api.Renderer(desc, W, H)
    L, ctx = r.L, r.ctx
    info = r.scene_info().as_dict()
    cdf = r.light_cdf()
    # materials in first-use order: 0 the lamp, 1 the floor's Lambertian, 2 the mirror, 3 the bare light; one texture
    for mat, t in ((1, 0), (2, 0), (-1, 0), (4, 0), (0, 1), (0, -2), (3, 7)):
        assert L.pt_set_material_emission_texture(ctx, mat, t) == PT_ERR_ARG, (mat, t)
    assert L.pt_set_material_texture(ctx, 0, 0) == PT_ERR_ARG and L.pt_set_material_texture(ctx, 3, 0) == PT_ERR_ARG   # lights: as ever
    assert L.pt_set_material_emission_texture(None, 0, 0) == PT_ERR_ARG
    assert r.scene_info().as_dict() == info
    now = r.light_cdf()                                                           # (PT_ERR_STATE if a refused call had un-built the scene)
    for k in ("pdf", "cdf", "blas", "prim"):
        assert_bit_equal(now[k], cdf[k], "light sampler after refused calls: " + k)
    # accepted calls un-build the scene
    assert L.pt_set_material_emission_texture(ctx, 3, 0) == 0
    n = C.c_uint32(); mx = C.c_float()
    assert L.pt_light_cdf(ctx, C.byref(n), None, None, None, None, C.byref(mx), 0) == PT_ERR_STATE
    r.rebuild()
    assert L.pt_set_material_emission_texture(ctx, 3, -1) == 0
    r.rebuild()
    for k in ("pdf", "cdf"):
        assert_bit_equal(r.light_cdf()[k], cdf[k], "set and cleared: " + k)


def test_light_cdf_is_the_restated_weights(api, oracle_mod):
    from path_tracer_amd.scene_desc import SceneDesc
    desc = _two_lights()
    r = api.Renderer(desc, W, H)
    orc = oracle_mod.Oracle(desc)                                                 # for the triangles' normals only: it knows nothing of textures
    n0 = lambda model, prim: orc.triangle(model, prim)[0:3]
    pdf, cdf, total = light_cdf(desc, n0)
    got = r.light_cdf()
    assert len(pdf) == 4 and pdf[0] != pdf[1] and pdf[2] == pdf[3]                # two lamp triangles of different weight, two equal bare ones
    assert_bit_equal(got["pdf"], pdf, "pdf"); assert_bit_equal(got["cdf"], cdf, "cdf")
    assert_bit_equal(np.array([got["max"]], F), np.array([total], F), "weight sum")
    # new UVs on the lamp move its weights, and only the sampler is rebuilt
    before = r.scene_info()
    uv = desc.models[0].uvs.copy(); uv[1] += F(0.37)
    r.set_model_uvs(0, uv); r.rebuild()
    lamp = copy.copy(desc.models[0]); lamp.uvs = uv
    moved = SceneDesc.new([lamp] + list(desc.models[1:]), desc.camera)
    pdf2, cdf2, _ = light_cdf(moved, n0)
    assert not np.array_equal(pdf2, pdf)
    assert_bit_equal(r.light_cdf()["cdf"], cdf2, "cdf after new UVs")
    after = r.scene_info()
    assert (after.blas_builds, after.tlas_builds) == (before.blas_builds, before.tlas_builds)


@pytest.mark.parametrize("walls", [True, False], ids=["textured walls", "emission texture only"])
def test_corner_scene_has_the_oracles_sampler(api, oracle_mod, walls):
    tex, plain = emission_corner_scene(W, H, wall_textures=walls)
    want = oracle_mod.Oracle(plain).light_cdf()
    got = api.Renderer(tex, W, H).light_cdf()
    assert len(want["cdf"]) == 2 * (N_LAMPS + 1)
    for k in ("pdf", "cdf", "blas", "prim"):
        assert_bit_equal(got[k], want[k], "corner scene sampler: " + k)
    assert_bit_equal(np.array([got["max"]], F), np.array([want["max"]], F), "weight sum")


def test_setter_rebuilds_the_sampler_and_nothing_else(api):
    from path_tracer_amd.scene_desc import SceneDesc
    tex, plain = emission_corner_scene(W, H)
    models = [copy.copy(m) for m in tex.models]
    for m in models[:N_LAMPS]:
        m.material = m.material.emission_textured(None)
    bare = SceneDesc.new(models, tex.camera)
    r = api.Renderer(bare, W, H)
    i0 = r.scene_info()
    cdf0 = r.light_cdf()["cdf"]
    tables = {w: (r.tlas_dump(w), r.tlas_instances(w)) for w in (0, 1)}
    lamp_tex = tex.models[0].material.emission_texture
    t = r.add_texture(lamp_tex.data)
    lamp_material = 0                                                             # the first material the description uses
    r.set_material_emission_texture(lamp_material, t); r.rebuild()
    i1 = r.scene_info()
    assert (i1.blas_builds, i1.tlas_builds) == (i0.blas_builds, i0.tlas_builds), i1.as_dict()
    assert not np.array_equal(r.light_cdf()["cdf"], cdf0)
    assert_bit_equal(r.light_cdf()["cdf"], api.Renderer(tex, W, H).light_cdf()["cdf"], "the sampler a fresh build has")
    for w in (0, 1):
        for have, was in zip((r.tlas_dump(w), r.tlas_instances(w)), tables[w]):
            for k in was:
                assert_bit_equal(np.asarray(have[k]), np.asarray(was[k]), f"tlas {w} {k}")


def test_emission_texture_alone_counts_as_a_textured_scene(api):
    desc = plumbing_scene(W, H)
    r = api.Renderer(desc, W, H)
    with_tex = r.scene_info().scene_bytes
    r.set_material_emission_texture(0, -1); r.rebuild()
    n_tris = 4
    assert with_tex == r.scene_info().scene_bytes + 24 * n_tris + 16 * 1 + 16 * 64


def test_a_sampler_without_weight_refuses_nee(api):
    from path_tracer_amd.scene_desc import Texture
    desc = plumbing_scene(W, H)
    black = desc.models[0].material.emission_textured(Texture.new(np.zeros((2, 2, 3), F)))
    desc.models[0].material = black
    r = api.Renderer(desc, W, H, enable_nee=True)
    assert not (r.light_cdf()["max"] > 0)
    o = np.zeros((1, 3), F); d = np.array([[0, -1, 0]], F)
    for call in (lambda: r.render(0, 1), lambda: r.render_samples(0, 1), lambda: r.integrate_rays(o, d, np.zeros(1, np.uint32), np.zeros(1, np.uint32))):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == PT_ERR_STATE and "no emissive model" in str(e.value)
    # a black light WITHOUT an emission texture is judged as ever: the call gets past this refusal (to the device, which this suite lacks)
    r.set_material_emission_texture(0, -1); r.rebuild()
    try:
        r.render(0, 1)
    except api.PtError as e:
        assert e.code != PT_ERR_STATE


def test_surface_colour_of_lights_on_the_host(api):
    desc = _two_lights()
    r = api.Renderer(desc, W, H)
    inst_model = world_instance_models(desc)
    rng = np.random.default_rng(21)
    n = 2000
    inst = rng.integers(0, len(inst_model), n).astype(np.uint32)
    ntri = np.array([desc.models[m].positions.shape[0] for m in inst_model])[inst]
    prim = (rng.integers(0, 1 << 30, n) % ntri).astype(np.uint32)
    u = rng.uniform(0.0, 1.0, n).astype(F)
    v = (rng.uniform(0.0, 1.0, n).astype(F) * (F(1.0) - u)).astype(F)
    got = r.surface_colour(inst, prim, u, v)
    want = scene_colour(desc, inst_model, inst, prim, u, v)
    assert_bit_equal(got, want, "surface colour, host")
    lamp = inst_model[inst] == 0
    assert lamp.sum() > 100 and len(np.unique(got[lamp], axis=0)) > 100           # the lamp's colour varies over it
    assert_bit_equal(got[inst_model[inst] == 3], np.broadcast_to(np.array([2.0, 3.0, 1.0], F), got[inst_model[inst] == 3].shape), "untextured light")


def test_plumbing_inputs_meet_their_conditions(api, oracle_mod):
    """the GPU suite's NEE-on plumbing test predicts zero / nonzero per sample; here, without a GPU: each class holds at least 20 % of the
    samples and at most 1 % are excluded as ambiguous"""
    pred = plumbing_classes(api, oracle_mod)
    n = pred.size
    assert (pred == 0).sum() >= 0.2 * n and (pred == 1).sum() >= 0.2 * n, np.bincount(pred.ravel(), minlength=3)
    assert (pred == 2).sum() <= 0.01 * n, np.bincount(pred.ravel(), minlength=3)


_PLUMB = {}


def plumbing_classes(api, oracle_mod):
    if "pred" not in _PLUMB:
        from path_tracer_amd.scene_desc import SceneDesc
        desc = plumbing_scene(W, H)
        orc = oracle_mod.Oracle(desc)
        white = oracle_mod.Oracle(SceneDesc.new([desc.models[1]], desc.camera))
        cdf = api.Renderer(desc, W, H).light_cdf()["cdf"]
        _PLUMB["pred"] = plumbing_prediction(desc, orc, white, cdf, W, H, SPP, oracle_mod.DEFAULT_SEED)
    return _PLUMB["pred"]


def test_dim_scene_stays_below_the_clamp_by_construction():
    """emission <= 4 and albedo 0.5: a path's radiance is below 4 * (1 + 0.5 + 0.25 + ...) = 8 whatever it does, far from the clamp at 100"""
    desc = dim_scene(W, H)
    assert desc.models[0].material.emission_texture.data.max() <= 4.0
    assert max(max(m.material.colour) for m in desc.models[1:]) <= 0.5
