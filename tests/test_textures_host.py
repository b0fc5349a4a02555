"""CPU: textures, UVs and the surface colour of include/pt_api.h without a GPU — the argument errors of the new entry points, the UVs the OBJ
reader keeps, pt_surface_colour's host evaluation against the numpy restatement of the definition (tests/textures_common.py), and what the
setters cost a build.  The renders are in tests/test_gpu_textures.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from textures_common import F, box, quad, scene_surface_colour, world_instance_models

NEW_SYMBOLS = ["pt_add_texture", "pt_set_material_texture", "pt_set_model_uvs", "pt_model_uvs", "pt_surface_colour", "pt_read_guide_albedo"]
PT_ERR_ARG, PT_ERR_STATE, PT_ERR_LIMIT = -1, -3, -5


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def test_new_symbols_exported_and_bound(api):
    L = C.CDLL(api._build.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(L, name), name
        assert getattr(api.lib(), name).argtypes is not None, name
    for meth in ("add_texture", "set_material_texture", "set_model_uvs", "model_uvs", "surface_colour", "read_guide_albedo"):
        assert callable(getattr(api.Renderer, meth)), meth
    assert C.sizeof(api.SceneInfo) == 64


def _desc(textured=True):
    """an instanced, tinted model with wild UVs on a 5 x 3 texture; an untinted model WITHOUT UVs on a 1 x 1; a tinted one on an 8 x 4; an
    untextured one; a light"""
    from path_tracer_amd.scene_desc import GGX, IDENTITY_3x4, Emissive, Lambertian, Model, SceneDesc, Texture
    rng = np.random.default_rng(3)
    t53 = Texture.new(rng.uniform(0.0, 2.0, (3, 5, 3)).astype(F))
    t11 = Texture.new(np.array([[[0.25, 0.5, 0.75]]], F))
    t84 = Texture.new(rng.uniform(0.0, 1.0, (4, 8, 3)).astype(F))
    tex = (lambda m, t: m.textured(t)) if textured else (lambda m, t: m)
    bp, bn = box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    uv = rng.uniform(-3.0, 3.0, (12, 3, 2)).astype(F)
    uv[0] = [[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]                                   # exactly 1.0
    uv[1] = [[-0.5, -2.0], [-1.0, -0.25], [-1e-9, -3.0]]                           # negative, and one that rounds up to 1.0 when wrapped
    uv[2] = [[1.0e6, 1.0e6 + 0.5], [1.0e6 + 3.0, 999999.25], [1000001.5, 1.0e6]]   # around 1e6
    uv[3] = [[0.2, 0.4], [0.2, 0.4], [0.2, 0.4]]                                   # all equal
    two = np.stack([IDENTITY_3x4, IDENTITY_3x4]); two[1, :, 3] = (5.0, 0.0, 0.0)
    qp, qn = quad((-9.0, -2.0, -9.0), (-9.0, -2.0, 9.0), (9.0, -2.0, 9.0), (9.0, -2.0, -9.0))
    lp, ln = quad((-1.0, 8.0, -1.0), (1.0, 8.0, -1.0), (1.0, 8.0, 1.0), (-1.0, 8.0, 1.0))
    models = [
        Model.new(bp, bn, tex(Lambertian.new((0.8, 0.6, 0.4)), t53), two, "instanced", uvs=uv),
        Model.new(qp, qn, tex(GGX.new_metal((1.0, 1.0, 1.0), 0.4), t11), None, "no uvs"),
        Model.new(lp, ln, Emissive.new((5.0, 5.0, 5.0)), None, "light"),
        Model.new(bp + F(20.0), bn, tex(Lambertian.new((0.3, 0.9, 0.5)), t84), None, "eight by four", uvs=rng.uniform(0.0, 1.0, (12, 3, 2)).astype(F)),
        Model.new(qp + F(0.5), qn, Lambertian.new((0.1, 0.2, 0.3)), None, "untextured", uvs=rng.uniform(0.0, 1.0, (2, 3, 2)).astype(F)),
    ]
    return SceneDesc.new(models, None, "surface colour")


def _queries(desc, n=4000):
    rng = np.random.default_rng(8)
    inst_model = world_instance_models(desc)
    inst = rng.integers(0, len(inst_model), n).astype(np.uint32)
    ntri = np.array([desc.models[m].positions.shape[0] for m in inst_model])[inst]
    prim = (rng.integers(0, 1 << 30, n) % ntri).astype(np.uint32)
    u = rng.uniform(0.0, 1.0, n).astype(F)
    v = (rng.uniform(0.0, 1.0, n).astype(F) * (F(1.0) - u)).astype(F)
    u[:6] = [0.0, 1.0, 0.0, 0.5, 0.25, 1.0]; v[:6] = [0.0, 0.0, 1.0, 0.5, 0.75, 0.0]   # the vertices and an edge
    # every special triangle of the instanced model is asked about, through both instances
    inst[6:14] = [0, 1, 0, 1, 0, 1, 0, 1]; prim[6:14] = [0, 0, 1, 1, 2, 2, 3, 3]
    return inst, prim, u, v


def test_surface_colour_on_the_host_is_the_definition(api):
    desc = _desc()
    r = api.Renderer(desc, 16, 16)
    inst, prim, u, v = _queries(desc)
    got = r.surface_colour(inst, prim, u, v)
    want = scene_surface_colour(desc, world_instance_models(desc), inst, prim, u, v)
    assert_bit_equal(got, want, "surface colour, host")
    models = world_instance_models(desc)[inst]
    assert_bit_equal(got[models == 2], np.broadcast_to(np.array([5.0, 5.0, 5.0], F), got[models == 2].shape), "emissive: the emitted colour")
    assert_bit_equal(got[models == 4], np.broadcast_to(np.array([0.1, 0.2, 0.3], F), got[models == 4].shape), "untextured: the colour, no arithmetic")
    assert_bit_equal(got[models == 1], np.broadcast_to(np.array([0.25, 0.5, 0.75], F), got[models == 1].shape), "1 x 1, untinted, no UVs")
    # the two consequences the header states: equal UVs are that UV everywhere; a power-of-two texel corner returns the texel
    t84 = desc.models[3].material.texture.data
    for (i, j) in ((0, 0), (7, 3), (3, 2), (5, 0)):
        r.set_model_uvs(3, np.broadcast_to(np.array([i / 8, j / 4], F), (12, 3, 2)))
        r.rebuild()
        sel = models == 3
        got = r.surface_colour(inst[sel], prim[sel], u[sel], v[sel])
        assert_bit_equal(got, np.broadcast_to(np.array([0.3, 0.9, 0.5], F) * t84[j, i], got.shape), f"texel corner {i},{j}")


def test_errors_are_refused_and_change_nothing(api):
    desc = _desc()
    r = api.Renderer(desc, 16, 16)
    L, ctx = r.L, r.ctx
    inst, prim, u, v = _queries(desc, 200)
    before = r.surface_colour(inst, prim, u, v)
    info = r.scene_info().as_dict()
    uv0 = r.model_uvs(0)
    good = np.ones((2, 2, 3), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def tex(w, h, a):
        return L.pt_add_texture(ctx, w, h, None if a is None else p(a))

    assert tex(0, 2, good) == PT_ERR_ARG and tex(2, 0, good) == PT_ERR_ARG and tex(2, 2, None) == PT_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf, -1e-30):
        a = good.copy(); a[1, 0, 2] = bad
        assert tex(2, 2, a) == PT_ERR_ARG, bad
    # (the other packing limit, 2^28 texels in all textures together, would take 3 GiB of host floats to reach: not exercised here)
    assert tex(16385, 1, np.ones((1, 16385, 3), F)) == PT_ERR_LIMIT and tex(1, 16385, np.ones((16385, 1, 3), F)) == PT_ERR_LIMIT
    n_tex = 3
    for mat, t in ((-1, 0), (99, 0), (0, n_tex), (0, -2), (2, 0)):                  # material 2 is the light's
        assert L.pt_set_material_texture(ctx, mat, t) == PT_ERR_ARG, (mat, t)
    uv = np.zeros((12, 3, 2), F)
    assert L.pt_set_model_uvs(ctx, -1, p(uv), 12) == PT_ERR_ARG and L.pt_set_model_uvs(ctx, 5, p(uv), 12) == PT_ERR_ARG
    assert L.pt_set_model_uvs(ctx, 0, p(uv), 11) == PT_ERR_ARG and L.pt_set_model_uvs(ctx, 0, None, 12) == PT_ERR_ARG
    assert L.pt_set_model_uvs(ctx, 0, p(uv), 0) == PT_ERR_ARG
    for bad in (np.nan, np.inf):
        a = uv.copy(); a[7, 1, 1] = bad
        assert L.pt_set_model_uvs(ctx, 0, p(a), 12) == PT_ERR_ARG
    n = C.c_uint32(77)
    assert L.pt_model_uvs(ctx, 9, None, 0, C.byref(n)) == PT_ERR_ARG and L.pt_model_uvs(ctx, 0, None, 0, None) == PT_ERR_ARG
    assert L.pt_model_uvs(ctx, 0, p(uv), 11, C.byref(n)) == PT_ERR_ARG and L.pt_model_uvs(ctx, 0, None, 12, C.byref(n)) == PT_ERR_ARG
    out = np.zeros((1, 3), F)
    one = lambda i, q: L.pt_surface_colour(ctx, 0, 1, p(np.array([i], np.uint32)), p(np.array([q], np.uint32)), p(np.zeros(1, F)), p(np.zeros(1, F)), p(out))
    assert one(6, 0) == PT_ERR_ARG and one(0, 12) == PT_ERR_ARG and one(2, 2) == PT_ERR_ARG
    assert L.pt_surface_colour(ctx, 0, 1, None, None, None, None, p(out)) == PT_ERR_ARG
    assert L.pt_read_guide_albedo(ctx, p(out)) == PT_ERR_STATE                      # no guides: nothing has touched a device
    # nothing changed: the scene is still built, counts, UVs and colours are what they were
    assert r.scene_info().as_dict() == info
    assert_bit_equal(r.model_uvs(0), uv0, "uvs after refused calls")
    assert_bit_equal(r.surface_colour(inst, prim, u, v), before, "surface colour after refused calls")
    # an accepted setter un-builds the scene
    r.set_material_texture(0, -1)
    assert L.pt_surface_colour(ctx, 0, 1, p(inst), p(prim), p(u), p(v), p(out)) == PT_ERR_STATE
    r.rebuild()
    sel = world_instance_models(desc)[inst] == 0
    assert_bit_equal(r.surface_colour(inst, prim, u, v)[sel], np.broadcast_to(np.array([0.8, 0.6, 0.4], F), (int(sel.sum()), 3)), "cleared")


OBJ = """# a quad (fan), a triangle with negative vt indices, one with an empty and a zero middle reference
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vn 0 0 1
vt 0.0 0.0
vt 1.0 0.0
vt 1.0 1.5
vt -0.25 1.0 0.0
f 1/1/1 2/2/1 3/3/1 4/4/1
f 1/-4/1 2/-1/1 3/-2/1
f 1//1 2/0/1 3/2/1
vt 0.5
f -4/5/-1 -3/-1/-1 -2/1/-1
"""


def test_uvs_round_trip_and_the_obj_reader_keeps_vt(api, tmp_path):
    from path_tracer_amd.scene_desc import Emissive, Lambertian, Model, SceneDesc
    with_vt = tmp_path / "uv.obj"
    with_vt.write_text(OBJ)
    without = tmp_path / "plain.obj"
    without.write_text("\n".join(l for l in OBJ.splitlines() if not l.startswith("vt")).replace("/1/", "//").replace("/2/", "//") + "\n")
    lp, ln = quad((-1.0, 8.0, -1.0), (1.0, 8.0, -1.0), (1.0, 8.0, 1.0), (-1.0, 8.0, 1.0))
    given = np.random.default_rng(2).uniform(-2.0, 2.0, (2, 3, 2)).astype(F)
    desc = SceneDesc.new([Model.from_obj(str(with_vt), Lambertian.new((0.5, 0.5, 0.5))), Model.from_obj(str(without), Lambertian.new((0.5, 0.5, 0.5))),
                          Model.new(lp, ln, Emissive.new((1.0, 1.0, 1.0)), uvs=given)])
    r = api.Renderer(desc, 8, 8)
    vt = {1: (0.0, 0.0), 2: (1.0, 0.0), 3: (1.0, 1.5), 4: (-0.25, 1.0), 5: (0.5, 0.0), 0: (0.0, 0.0)}
    want = np.array([[vt[1], vt[2], vt[3]], [vt[1], vt[3], vt[4]],          # the fan of the quad
                     [vt[1], vt[4], vt[3]],                                # -4, -1, -2 of four
                     [vt[0], vt[0], vt[2]],                                # empty, 0, 2
                     [vt[5], vt[5], vt[1]]], F)                            # after the fifth vt: 5, -1, 1
    p, _ = r.model_vertices(0)
    assert p.shape[0] == 5
    assert_bit_equal(r.model_uvs(0), want, "uvs of the OBJ")
    assert r.model_uvs(1) is None and r.model_vertices(1)[0].shape[0] == 5
    assert_bit_equal(r.model_uvs(2), given, "uvs as set")
    r.set_model_uvs(2, None)
    assert r.model_uvs(2) is None
    r.set_model_uvs(1, want)
    assert_bit_equal(r.model_uvs(1), want, "uvs set on an OBJ model")
    n = C.c_uint32(0)
    assert r.L.pt_model_uvs(r.ctx, 1, None, 0, C.byref(n)) == 0 and n.value == 5


def test_texture_edits_build_no_blas_and_no_tlas(api):
    desc = _desc()
    r = api.Renderer(desc, 16, 16)
    n_models = len(desc.models)
    i0 = r.scene_info()
    assert (i0.blas_builds, i0.tlas_builds) == (n_models, 1)
    tables = {w: (r.tlas_dump(w), r.tlas_instances(w)) for w in (0, 1)}
    r.set_material_texture(0, 2); r.rebuild()
    r.set_model_uvs(3, np.zeros((12, 3, 2), F)); r.rebuild()
    r.set_model_uvs(1, None); r.set_material_texture(1, -1); r.rebuild()
    t = r.add_texture(np.ones((3, 2, 3), F)); r.set_material_texture(4, t); r.rebuild()
    i1 = r.scene_info()
    assert (i1.blas_builds, i1.tlas_builds) == (n_models, 1), i1.as_dict()
    for w in (0, 1):
        for have, was in zip((r.tlas_dump(w), r.tlas_instances(w)), tables[w]):
            for k in was:
                assert_bit_equal(np.asarray(have[k]), np.asarray(was[k]), f"tlas {w} {k}")
    inst, prim, u, v = _queries(desc, 300)
    sel = world_instance_models(desc)[inst] == 4
    assert_bit_equal(r.surface_colour(inst, prim, u, v)[sel], np.broadcast_to(np.array([0.1, 0.2, 0.3], F), (int(sel.sum()), 3)), "white texture")
    # a move afterwards rebuilds the TLASes as it always did
    m = desc.models[3].matrices.copy(); m[0, :, 3] += F(1.0)
    r.set_instances(3, m); r.rebuild()
    assert r.scene_info().tlas_builds == 2 and r.scene_info().blas_builds == n_models


def test_unreferenced_textures_and_uvs_cost_the_flattened_scene_nothing(api):
    plain = api.Renderer(_desc(textured=False), 16, 16)
    for i in range(5):
        plain.set_model_uvs(i, None)
    plain.rebuild()
    base = plain.scene_info().scene_bytes
    assert base > 0
    r = api.Renderer(_desc(textured=False), 16, 16)                       # UVs set (by the description), textures added, none referenced
    r.add_texture(np.ones((4, 8, 3), F)); r.add_texture(np.ones((1, 1, 3), F))
    r.rebuild()
    assert r.scene_info().scene_bytes == base
    r.set_material_texture(0, 0); r.rebuild()
    n_tris = 12 + 2 + 2 + 12 + 2
    assert r.scene_info().scene_bytes == base + 24 * n_tris + 16 * 2 + 16 * (32 + 1)
    r.set_material_texture(0, -1); r.rebuild()
    assert r.scene_info().scene_bytes == base
