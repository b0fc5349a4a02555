"""CPU: roughness maps (pt_set_material_roughness_texture, include/pt_api.h) without a GPU: the setter's refusals, what it costs a build and
a flatten, pt_surface_roughness's host evaluation against the numpy restatement of the definition (tests/roughness_common.py), constant maps,
and the conditions of the GPU tests' scenes, asserted from the oracle's side alone.  The renders are in tests/test_gpu_roughness.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import roughness_common as RC
from conftest import assert_bit_equal
from roughness_common import F
from textures_common import bilinear, world_instance_models

PT_ERR_ARG, PT_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def test_new_symbols_exported_and_declared(api):
    import os
    from conftest import ROOT
    L = C.CDLL(api._build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in ("pt_set_material_roughness_texture", "pt_surface_roughness"):
        assert name in api.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    assert callable(api.Renderer.set_material_roughness_texture) and callable(api.Renderer.surface_roughness)
    assert "roughness maps (normal maps" not in header and "roughness / height" not in header, "no out-of-scope list names them any more"


def test_the_description_takes_a_map_on_ggx_only():
    from path_tracer_amd.scene_desc import GGX, Dielectric, Emissive, Lambertian, Specular
    t = RC.constant_map(2, 2, 0.5)
    for m in (GGX.new_metal((1, 1, 1), 0.3), GGX.new_dielectric((1, 1, 1), 0.3, 1.5)):
        assert m.roughness_mapped(t).roughness_texture is t and m.roughness_mapped(t).roughness_mapped(None) == m
        assert m.roughness_mapped(t).textured(t).normal_mapped(t).roughness_texture is t
    for m in (Lambertian.new((1, 1, 1)), Emissive.new((1, 1, 1)), Specular.new((1, 1, 1)), Dielectric.new((1, 1, 1), 1.5)):
        with pytest.raises(ValueError):
            m.roughness_mapped(t)


# ---- 1. errors
def test_errors_are_refused_and_change_nothing(api):
    from path_tracer_amd.scene_desc import Dielectric, Emissive, GGX, Lambertian, Model, SceneDesc, Specular
    from textures_common import quad
    qp, qn = quad((-1.0, 0.0, -1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, -1.0))
    kinds = [GGX.new_metal((0.9, 0.8, 0.7), 0.3).roughness_mapped(RC.varied_map(5, 3, 1)), Emissive.new((5.0, 5.0, 5.0)), Lambertian.new((0.5, 0.5, 0.5)),
             Specular.new((0.9, 0.9, 0.9)), Dielectric.new((1.0, 1.0, 1.0), 1.5), GGX.new_dielectric((1.0, 1.0, 1.0), 0.2, 1.5)]
    desc = SceneDesc.new([Model.new(qp + F(3.0 * k), qn, m, None, f"m{k}", uvs=np.random.default_rng(k).uniform(0, 1, (2, 3, 2)).astype(F))
                          for k, m in enumerate(kinds)], None, "kinds")
    r = api.Renderer(desc, 16, 16)
    L, ctx = r.L, r.ctx
    q = RC.hook_queries(desc, 200)
    before = r.surface_roughness(*q)
    assert_bit_equal(before, RC.scene_alpha(desc, *q), "the kinds' alphas")
    info = r.scene_info().as_dict()
    n_tex = 1
    for mat, t in ((-1, 0), (99, 0), (len(kinds), 0), (0, n_tex), (0, -2), (1, 0), (1, -1), (2, 0), (2, -1), (3, 0), (4, 0), (4, -1)):
        assert L.pt_set_material_roughness_texture(ctx, mat, t) == PT_ERR_ARG, (mat, t)
    out = np.zeros(1, F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    z = np.zeros(1, F)
    one = lambda i, k: L.pt_surface_roughness(ctx, 0, 1, p(np.array([i], np.uint32)), p(np.array([k], np.uint32)), p(z), p(z), p(out))
    assert one(len(kinds), 0) == PT_ERR_ARG and one(0, 2) == PT_ERR_ARG
    assert L.pt_surface_roughness(ctx, 0, 1, None, None, None, None, p(out)) == PT_ERR_ARG
    assert L.pt_surface_roughness(ctx, 0, 1, p(np.zeros(1, np.uint32)), p(np.zeros(1, np.uint32)), p(z), p(z), None) == PT_ERR_ARG
    assert r.scene_info().as_dict() == info                                           # still built, same bytes, same build counters
    assert_bit_equal(r.surface_roughness(*q), before, "alphas after refused calls")
    # an accepted setter un-builds the scene; the GGX dielectric takes the map too, and clearing restores the materials' own alphas
    r.set_material_roughness_texture(5, 0)
    assert one(0, 0) == PT_ERR_STATE
    r.rebuild()
    both = SceneDesc.new(desc.models[:5] + [dataclasses.replace(desc.models[5], material=kinds[5].roughness_mapped(kinds[0].roughness_texture))], None, "both")
    assert_bit_equal(r.surface_roughness(*q), RC.scene_alpha(both, *q), "both GGX kinds mapped")
    r.set_material_roughness_texture(0, -1); r.set_material_roughness_texture(5, -1); r.rebuild()
    assert_bit_equal(r.surface_roughness(*q), RC.scene_alpha(RC.untextured(desc), *q), "cleared: the materials' own alphas")


# ---- 2. build and flatten
def test_the_setter_builds_nothing_and_a_move_afterwards_rebuilds_no_blas(api):
    desc = RC.hook_scene()
    r = api.Renderer(desc, 16, 16)
    n_models = len(desc.models)
    i0 = r.scene_info()
    assert (i0.blas_builds, i0.tlas_builds) == (n_models, 1)
    tables = {w: (r.tlas_dump(w), r.tlas_instances(w)) for w in (0, 1)}
    t = r.add_texture(RC.constant_map(2, 2, 0.5).data)
    r.set_material_roughness_texture(4, t); r.rebuild()                              # the unmapped GGX quad's material
    r.set_material_roughness_texture(0, -1); r.rebuild()
    r.set_material_roughness_texture(0, 1); r.rebuild()
    i1 = r.scene_info()
    assert (i1.blas_builds, i1.tlas_builds) == (n_models, 1), i1.as_dict()
    for w in (0, 1):
        for have, was in zip((r.tlas_dump(w), r.tlas_instances(w)), tables[w]):
            for k in was:
                assert_bit_equal(np.asarray(have[k]), np.asarray(was[k]), f"tlas {w} {k}")
    m = desc.models[3].matrices.copy(); m[0, :, 3] += F(1.0)
    r.set_instances(3, m); r.rebuild()
    assert r.scene_info().tlas_builds == 2 and r.scene_info().blas_builds == n_models


def test_a_map_makes_a_textured_scene_and_clearing_gives_the_bytes_of_a_scene_never_mapped(api):
    from path_tracer_amd.scene_desc import SceneDesc
    desc = RC.hook_scene()
    # a scene whose ONLY textures are roughness maps: UVs, table and texels come with the first reference and go with the last
    only = SceneDesc.new([dataclasses.replace(m, material=m.material.textured(None)) if m.material.kind != 1 else m for m in desc.models], None, "only maps")
    never = RC.untextured_roughness(only)
    assert all(m.material.texture is None and m.material.roughness_texture is None for m in never.models)
    rn = api.Renderer(never, 16, 16)
    b0 = rn.scene_info().scene_bytes
    ro = api.Renderer(only, 16, 16)
    n_tris = 12 + 2 + 2 + 12 + 2 + 2
    texels = 5 * 3 + 1 + 8 * 4
    assert ro.scene_info().scene_bytes == b0 + 24 * n_tris + 16 * 3 + 16 * texels, "has_textures: the UVs, the table and the texels"
    # the texels stay in the scene, referenced by nobody: the flattened scene is the one that never had a map
    for m in (0, 1, 3):
        rn.add_texture(only.models[m].material.roughness_texture.data)
    rn.rebuild()
    assert rn.scene_info().scene_bytes == b0
    for mi in sorted({ro._materials.index(m.material) for m in only.models if m.material.roughness_texture is not None}):
        ro.set_material_roughness_texture(mi, -1)
    ro.rebuild()
    assert ro.scene_info().scene_bytes == b0
    q = RC.hook_queries(desc, 300)
    assert_bit_equal(ro.surface_roughness(*q), rn.surface_roughness(*q), "cleared: the scene never mapped")
    assert_bit_equal(ro.surface_roughness(*q), RC.scene_alpha(never, *q), "... which is the materials' own alphas")


# ---- 3. the host evaluation is the definition
def test_surface_roughness_on_the_host_is_the_definition(api):
    desc = RC.hook_scene()
    r = api.Renderer(desc, 16, 16)
    q = RC.hook_queries(desc)
    inst, prim = q[0], q[1]
    got = r.surface_roughness(*q)
    assert_bit_equal(got, RC.scene_alpha(desc, *q), "surface roughness, host")
    models = world_instance_models(desc)[inst]
    assert set(np.unique(models).tolist()) == set(range(len(desc.models))), "every model is asked about"
    assert (got[(models == 2) | (models == 5)] == 0).all(), "the light and the Lambertian quad: not GGX"
    un = got[models == 4]
    rough = F(RC.UNMAPPED_ROUGHNESS)
    assert (un.view(np.uint32) == RC.clamp_alpha(rough * rough).view(np.uint32)).all() and len(un), "unmapped: clamp(sq(f32 roughness))"
    one = got[models == 1]
    assert (one.view(np.uint32) == RC.clamp_alpha(F(0.55) * F(0.55)).view(np.uint32)).all() and len(one), "no UVs under a 1 x 1 map: its texel"
    big = got[models == 3]
    assert (big == F(1e-4)).any() and (big == F(0.9999)).any(), "both clamps are reached on the 8 x 4 map"
    assert len(np.unique(got[models == 0])) > 500, "the 5 x 3 map is interpolated"
    # the map is read, not the material: no mapped hit (away from the clamps' coincidences) keeps the material's own alpha
    assert (got[models == 0] != RC.material_alpha(0.3)).all()


def test_a_constant_map_is_the_material_of_that_roughness_everywhere(api):
    """a constant 5 x 3 map of rho under the hook scene's UVs (mirrored, negative, exactly 1, 1e6): clamp(rho * rho), bit for bit, at every
    query, although a plain bilinear blend of four equal texels is an ulp off at some of them"""
    from path_tracer_amd.scene_desc import GGX
    rho = 0.45
    tex = RC.constant_map(5, 3, rho)
    desc = RC.hook_scene(t53=tex)
    r = api.Renderer(desc, 16, 16)
    q = RC.hook_queries(desc)
    inst, prim, u, v = q
    sel = world_instance_models(desc)[inst] == 0
    got = r.surface_roughness(*q)[sel]
    want = RC.clamp_alpha(F(rho) * F(rho))
    assert sel.sum() > 500 and (got.view(np.uint32) == want.view(np.uint32)).all()
    assert_bit_equal(got, np.full(int(sel.sum()), RC.material_alpha(rho), F), "GGX::new_metal(.., rho)")
    # the four-equal exception is exercised: the plain blend would be off somewhere
    uv3 = np.asarray(desc.models[0].uvs, F)[prim[sel]]
    s, t = RC.hit_st(uv3, u[sel], v[sel])
    blend = bilinear(tex.data, s, t)[:, 0]
    off = blend != F(rho)
    assert off.any(), "choose rho and UVs so that a plain blend is an ulp off somewhere"
    assert (np.abs(blend[off].astype(np.float64) - float(F(rho))) < 1e-6).all()
    x = blend * blend
    assert (RC.clamp_alpha(x).view(np.uint32) != want.view(np.uint32)).any(), "... and so would its alpha"


def test_texel_corners_read_that_texel(api):
    """at s = i / w, t = j / h (w and h powers of two) the alpha is texel (i, j)'s: the corner room's models"""
    mapped, plain = RC.corner_room(32, 24)
    r = api.Renderer(mapped, 32, 24)
    q = RC.hook_queries(mapped, 500)
    got = r.surface_roughness(*q)
    assert_bit_equal(got, RC.scene_alpha(mapped, *q), "corner room, restated")
    assert_bit_equal(got, RC.scene_alpha(plain, *q), "corner room: the equivalent's own alphas")
    names = {m.name: m.material.roughness for m in plain.models}
    want = {"block": RC.R22[(0, 0)], "slab": RC.R22[(1, 0)], "glass_a": RC.R22[(1, 1)], "glass_b": RC.R22[(0, 1)]}
    for n, rr in want.items():
        assert names[n] == float(F(rr)), (n, names[n], rr)
    assert 0.35 not in want.values() and 0.2 not in want.values()


# ---- 4. the conditions of the GPU tests' varying-map composition, from the oracle's side alone
def test_the_varying_maps_conditions_hold(oracle_mod):
    import test_gpu_roughness as TG
    for kind in ("metal", "dielectric"):
        desc = TG.varying_quad(kind)
        orc = oracle_mod.Oracle(RC.untextured(desc))
        hits = TG.quad_hits(orc, desc)
        assert len(hits["rho"]) > TG.QW * TG.QH * TG.QSPP // 3, "more than a third of the samples hit the quad"
        assert (hits["rho"] != F(0.35)).all(), "every quad hit's rho differs from the material's own"
        texels = desc.models[0].material.roughness_texture.data[..., 0].reshape(-1)
        assert not np.isin(hits["rho"], texels).any(), "every quad hit's rho is truly interpolated"
        assert hits["rho"].min() >= F(0.1) and hits["rho"].max() <= F(0.9)


@pytest.mark.parametrize("nee", [False, True], ids=["no_nee", "nee"])
@pytest.mark.parametrize("kind", ["metal", "dielectric"])
def test_the_composition_at_the_materials_own_roughness_is_the_oracles_integrate(oracle_mod, kind, nee):
    """tests/test_gpu_roughness.py predicts a roughness-mapped quad's samples by shading every hit with an oracle whose material has the hit's
    rho.  Under a constant map of the material's own 0.35 that composition must be the oracle's render of the unmapped quad, bit for bit, for
    the metal and for the dielectric (which tests/test_normalmap_host.py does not compose): what the GPU test adds is rho alone."""
    import test_gpu_roughness as TG
    desc = TG.varying_quad(kind, RC.constant_map(5, 3, 0.35))
    want, hits, orc = TG.composed(oracle_mod, desc, nee)
    assert len(hits["rho"]) > TG.QW * TG.QH * TG.QSPP // 3 and (hits["rho"] == F(0.35)).all()
    assert_bit_equal(want, orc.render_samples(TG.QW, TG.QH, TG.QSPP, max_bounces=1, enable_nee=int(nee)), f"{kind}, nee {nee}")


# ---- the host-sanitizer build (make host-asan: the stand-alone CPU program of path_tracer_amd/csrc/host_sanitize.cpp) is driven by
# tests/test_roughness_host_sanitizer.py
