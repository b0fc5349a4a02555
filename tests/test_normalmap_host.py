"""CPU: normal maps (pt_set_material_normal_texture, include/pt_api.h) without a GPU — the argument errors, pt_shading_normal's host evaluation
against the numpy restatement of the definition (tests/normalmap_common.py), and what the setter costs a build.  The renders are in
tests/test_gpu_normalmap.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from normalmap_common import F, encode, hook_queries, hook_scene, scene_shading_normal, tangents
from textures_common import world_instance_models

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
    for name in ("pt_set_material_normal_texture", "pt_shading_normal"):
        assert name in api.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    assert callable(api.Renderer.set_material_normal_texture) and callable(api.Renderer.shading_normal)


def _restated(r, desc, q):
    t = r.tlas_instances(0)
    return scene_shading_normal(desc, t["matrix"], t["inv_matrix"], *q)


# ---- 1. errors
def test_errors_are_refused_and_change_nothing(api):
    from path_tracer_amd.scene_desc import Emissive, Lambertian, Model, SceneDesc, Texture
    from textures_common import quad
    desc = hook_scene()
    r = api.Renderer(desc, 16, 16)
    L, ctx = r.L, r.ctx
    q = hook_queries(desc, 200)
    before = r.shading_normal(*q)
    info = r.scene_info().as_dict()
    n_tex, light = 4, 2                                                               # material 2 is the light's
    for mat, t in ((-1, 0), (99, 0), (0, n_tex), (0, -2), (light, 0), (light, -1)):
        assert L.pt_set_material_normal_texture(ctx, mat, t) == PT_ERR_ARG, (mat, t)
    out = np.zeros((1, 3), F); fr = np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    z = np.zeros(1, F); d = np.array([[0.0, -1.0, 0.0]], F)
    one = lambda i, k: L.pt_shading_normal(ctx, 0, 1, p(np.array([i], np.uint32)), p(np.array([k], np.uint32)), p(z), p(z), p(d), p(out), p(fr))
    assert one(6, 0) == PT_ERR_ARG and one(0, 12) == PT_ERR_ARG and one(2, 2) == PT_ERR_ARG
    assert L.pt_shading_normal(ctx, 0, 1, None, None, None, None, None, p(out), p(fr)) == PT_ERR_ARG
    assert r.scene_info().as_dict() == info                                           # still built, same bytes, same build counters
    got = r.shading_normal(*q)
    assert_bit_equal(got[0], before[0], "normals after refused calls"); assert np.array_equal(got[1], before[1])
    # a light with an emission texture refuses a normal texture like any light
    lp, ln = quad((-1.0, 8.0, -1.0), (1.0, 8.0, -1.0), (1.0, 8.0, 1.0), (-1.0, 8.0, 1.0))
    lamp = Emissive.new((5.0, 5.0, 5.0)).emission_textured(Texture.new(np.ones((2, 2, 3), F)))
    e = api.Renderer(SceneDesc.new([Model.new(lp, ln, lamp, None, "lamp"), Model.new(lp - F(3.0), ln, Lambertian.new((0.5, 0.5, 0.5)))]), 8, 8)
    einfo = e.scene_info().as_dict()
    assert e.L.pt_set_material_normal_texture(e.ctx, 0, 0) == PT_ERR_ARG
    assert e.scene_info().as_dict() == einfo
    # an accepted setter un-builds the scene
    r.set_material_normal_texture(0, -1)
    assert one(0, 0) == PT_ERR_STATE


def test_clearing_gives_the_bytes_of_a_scene_never_mapped(api):
    from path_tracer_amd.scene_desc import SceneDesc
    desc = hook_scene()
    # the same scene without any normal map (the colour texture of model 3 stays)
    import dataclasses
    never = SceneDesc.new([dataclasses.replace(m, material=m.material.normal_mapped(None)) for m in desc.models], None, "never mapped")
    rb = api.Renderer(never, 16, 16)
    for m in (0, 1, 3):                                                                # the maps' texels are in the scene, referenced by nobody
        rb.add_texture(desc.models[m].material.normal_texture.data)
    rb.rebuild()
    base = rb.scene_info().scene_bytes
    r = api.Renderer(desc, 16, 16)
    n_tris = 12 + 2 + 2 + 12 + 2
    assert r.scene_info().scene_bytes == base + 16 * n_tris                            # the tangents; UVs and texels are there for the colour texture
    mats = sorted({r._materials.index(m.material) for m in desc.models if m.material.normal_texture is not None})
    for mi in mats:
        r.set_material_normal_texture(mi, -1)
    r.rebuild()
    assert r.scene_info().scene_bytes == base
    q = hook_queries(desc, 300)
    got = r.shading_normal(*q)
    want = _restated(r, never, q)
    assert_bit_equal(got[0], want[0], "cleared: the plain normal"); assert np.array_equal(got[1], want[1])
    # a scene whose ONLY textures are normal maps: UVs, table and texels come with the first reference and go with the last
    only = SceneDesc.new([dataclasses.replace(m, material=m.material.textured(None)) if m.material.kind != 1 else m for m in desc.models], None, "only maps")
    plain = SceneDesc.new([dataclasses.replace(m, material=m.material.normal_mapped(None)) for m in only.models], None, "no texture at all")
    b0 = api.Renderer(plain, 16, 16).scene_info().scene_bytes
    ro = api.Renderer(only, 16, 16)
    texels = 5 * 3 + 1 + 8 * 4
    assert ro.scene_info().scene_bytes == b0 + (24 + 16) * n_tris + 16 * 3 + 16 * texels


# ---- 2. the host evaluation is the definition
def test_shading_normal_on_the_host_is_the_definition(api):
    desc = hook_scene()
    r = api.Renderer(desc, 16, 16)
    q = hook_queries(desc)
    inst, prim = q[0], q[1]
    got, front = r.shading_normal(*q)
    want, wfront = _restated(r, desc, q)
    assert np.array_equal(front, wfront)
    assert_bit_equal(got, want, "shading normal, host")
    assert front.min() == 0 and front.max() == 1, "front and back faces"
    # what the cases were meant to cover is covered
    tan, sign = tangents(desc.models[0].positions, desc.models[0].uvs)
    assert sign[5] == -sign[6] and (tan[3] == 0).all() and (tan[4] == 0).all() and sign[3] == 1 and (tan[5] != 0).any()
    models = world_instance_models(desc)[inst]
    plain = api.Renderer(hook_scene(flat=True), 16, 16)
    pn, pf = plain.shading_normal(*q)
    assert np.array_equal(pf, front), "front is the unperturbed normal's flag"
    keeps = (models == 1) | (models == 2) | (models == 4) | ((models == 0) & ((prim == 3) | (prim == 4)))
    assert_bit_equal(got[keeps], pn[keeps], "no UVs, degenerate UVs, the light, the unmapped model: the plain normal")
    moved = ~keeps
    assert (np.abs(got[moved] - pn[moved]).max(axis=1) > 1e-3).mean() > 0.95, "the map perturbs everything else"
    assert np.allclose(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)), 1.0, atol=1e-5)


def test_a_flat_texel_returns_the_plain_normal_everywhere(api):
    """texels of exactly (0.5, 0.5, 1.0), on 1 x 1, 5 x 3 and 8 x 4 maps: hit_normal's value, bit for bit, for every case of the test above"""
    import dataclasses
    from path_tracer_amd.scene_desc import SceneDesc
    desc = hook_scene(flat=True)
    r = api.Renderer(desc, 16, 16)
    q = hook_queries(desc)
    got, front = r.shading_normal(*q)
    never = SceneDesc.new([dataclasses.replace(m, material=m.material.normal_mapped(None)) for m in desc.models], None, "never mapped")
    rn = api.Renderer(never, 16, 16)
    want, wfront = rn.shading_normal(*q)                                               # no normal texture: the plain path of the same function
    assert_bit_equal(got, want, "flat maps"); assert np.array_equal(front, wfront)
    rest, rfront = _restated(rn, never, q)                                             # ... which is hit_normal as restated
    assert_bit_equal(want, rest, "the plain normal is the restated one"); assert np.array_equal(wfront, rfront)
    assert_bit_equal(encode([0.0, 0.0, 1.0]), np.array([0.5, 0.5, 1.0], F), "the flat texel")


# ---- 3. counters
def test_the_setter_builds_nothing_and_a_move_afterwards_is_patched(api):
    desc = hook_scene()
    r = api.Renderer(desc, 16, 16)
    n_models = len(desc.models)
    i0 = r.scene_info()
    assert (i0.blas_builds, i0.tlas_builds) == (n_models, 1)
    epoch_tables = {w: (r.tlas_dump(w), r.tlas_instances(w)) for w in (0, 1)}
    t = r.add_texture(encode(np.broadcast_to(np.array([0.6, 0.0, 0.8], F), (2, 2, 3))))
    r.set_material_normal_texture(4, t); r.rebuild()
    r.set_material_normal_texture(0, -1); r.rebuild()
    r.set_material_normal_texture(0, 1); r.rebuild()
    i1 = r.scene_info()
    assert (i1.blas_builds, i1.tlas_builds) == (n_models, 1), i1.as_dict()
    for w in (0, 1):
        for have, was in zip((r.tlas_dump(w), r.tlas_instances(w)), epoch_tables[w]):
            for k in was:
                assert_bit_equal(np.asarray(have[k]), np.asarray(was[k]), f"tlas {w} {k}")
    # a move afterwards rebuilds the TLASes as it always did and no BLAS
    m = desc.models[3].matrices.copy(); m[0, :, 3] += F(1.0)
    r.set_instances(3, m); r.rebuild()
    assert r.scene_info().tlas_builds == 2 and r.scene_info().blas_builds == n_models
    # (that the upload after the setter is a full one and the move's a patch needs a device: tests/test_gpu_normalmap.py)


# ---- the GPU tests' composition from oracle pieces, checked here against the oracle itself
@pytest.mark.parametrize("nee", [False, True], ids=["no_nee", "nee"])
@pytest.mark.parametrize("kind", ["lambertian", "specular", "ggx_metal"])
def test_the_composition_with_the_plain_normal_is_the_oracles_integrate(api, oracle_mod, kind, nee):
    """tests/test_gpu_normalmap.py predicts the samples of a normal-mapped quad from oracle pieces: one bounce and, with NEE on, both direct-light
    estimates restated around pt_bsdf_eval and pt_material_eval (normalmap_common.composed_samples).  Fed the oracle's OWN normal instead of N',
    that composition must be the oracle's integrate(), bit for bit: the restatement of the estimates, their draws and their order is then right,
    and what the GPU test adds is N' alone."""
    import dataclasses
    from path_tracer_amd.scene_desc import GGX, Lambertian, SceneDesc, Specular
    from normalmap_common import composed_samples, quad_scene
    material = dict(lambertian=Lambertian.new((0.9, 0.8, 0.7)), specular=Specular.new((0.9, 0.85, 0.8)),
                    ggx_metal=GGX.new_metal((0.9, 0.75, 0.6), 0.35))[kind]
    w = h = 8
    desc = quad_scene(w, h, material)
    t = api.Renderer(desc, w, h, max_bounces=1).tlas_instances(0)
    got, n_quad, _ = composed_samples(oracle_mod, desc, t["matrix"], t["inv_matrix"], w, h, 2, nee, mapped=False)
    plain = dataclasses.replace(desc.models[0], material=material, uvs=None)
    want = oracle_mod.Oracle(SceneDesc.new([plain] + list(desc.models[1:]), desc.camera)).render_samples(w, h, 2, max_bounces=1, enable_nee=int(nee))
    assert n_quad > w * h * 2 // 3
    assert_bit_equal(got, want, f"{kind}, nee {nee}: the composition with the plain normal")
    if nee and kind != "specular":
        lit = got[..., :3].max(axis=-1) > 0.05                                          # the small light reaches most of the diffuse quad;
        assert lit.mean() > (0.5 if kind == "lambertian" else 0.05)                     # the glossy lobe finds it from a few pixels only
        mapped, _, moved = composed_samples(oracle_mod, desc, t["matrix"], t["inv_matrix"], w, h, 2, nee)
        assert moved == n_quad and (mapped != got).any(axis=-1).sum() >= n_quad * 9 // 10, "N' changes the direct light nearly everywhere"


# ---- the host-sanitizer build (make host-asan: the stand-alone CPU program of path_tracer_amd/csrc/host_sanitize.cpp) over the new host code
def test_tangents_and_the_host_evaluation_under_the_host_sanitizers():
    import json
    import os
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "path_tracer_amd", "csrc")
    b = subprocess.run(["make", "-C", csrc, "host-asan"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([os.path.join(ROOT, "path_tracer_amd", "host_sanitize"), "normals", "500", "7"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["triangles"] == 500 and 250 <= res["with_tangent"] <= 300, res          # two shapes in five are degenerate
