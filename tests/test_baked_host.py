"""CPU: lightmaps kept by the context and the baked view (pt_set_lightmap, pt_get_lightmap_info, pt_lightmap_lookup, pt_render_baked) without a
GPU: the symbols, every refusal include/pt_api.h promises before any device call with "nothing changed" checked, the host evaluation of the
lookup against the numpy restatement of tests/baked_common.py bit for bit, its two exact cases, the round trip with the bake's texel
convention, and the maps' lifetime.  No GPU is touched (the device lookup and the view itself: tests/test_gpu_baked.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import baked_common as BC
import lightmap_common as LC
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, STATE, LIMIT = -1, -3, -5
NEW_SYMBOLS = ["pt_set_lightmap", "pt_get_lightmap_info", "pt_lightmap_lookup", "pt_render_baked", "pt_read_baked", "pt_reset_baked", "pt_write_baked_image"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _info(r):
    return r.scene_info().as_dict()


def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert "typedef struct pt_baked_params" in header
    for method in ("set_lightmap", "set_lightmap_sums", "lightmap_info", "lightmap_lookup", "render_baked", "read_baked", "reset_baked", "write_baked_image"):
        assert callable(getattr(api.Renderer, method))
    assert C.sizeof(api.BakedParams) == 32
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for word in ("set_lightmap(", "lightmap_info(", "lightmap_lookup(", "render_baked(", "read_baked(", "reset_baked(", "write_baked_image("):
        assert word in wrapper, word
    assert "feeding a baked map back" not in header


def test_set_lightmap_refusals_change_nothing(api):
    sc, model = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)
    good = np.random.default_rng(1).uniform(0, 1, (3, 5, 3)).astype(F)
    r.set_lightmap(model, 0, good)
    assert r.lightmap_info(model, 0) == (5, 3)
    inst, prim, u, v = np.zeros(4, np.uint32) + model, np.arange(4, dtype=np.uint32), np.full(4, 0.25, F), np.full(4, 0.5, F)
    before, info = r.lightmap_lookup(inst, prim, u, v), _info(r)
    L, small = r.L, np.ones((2, 2, 3), F)

    def bad(value):
        a = small.copy()
        a[1, 0, 2] = value
        return a
    one = np.zeros(3, F)        # never read past its sizes: each of these is refused for its sizes alone
    refusals = [
        ((-1, 0, 2, 2, small), ARG), ((len(sc.models), 0, 2, 2, small), ARG), ((model, 1, 2, 2, small), ARG),
        ((model, 0, 0, 2, small), ARG), ((model, 0, 2, 0, small), ARG), ((model, 0, 0, 0, small), ARG),
        ((model, 0, 2, 2, None), ARG), ((model, 0, 2, 0, None), ARG), ((model, 0, 0, 2, None), ARG),
        ((model, 0, 2, 2, bad(-1e-30)), ARG), ((model, 0, 2, 2, bad(np.nan)), ARG), ((model, 0, 2, 2, bad(np.inf)), ARG),
        ((0, 0, 2, 2, small), STATE),                                              # cb_light carries no UVs
        ((model, 0, 16385, 1, one), LIMIT), ((model, 0, 1, 16385, one), LIMIT),
        # where several apply: indices and sizes, then the limits, then the UVs, the texels last (include/pt_api.h)
        ((0, 0, 16385, 1, one), LIMIT), ((0, 0, 2, 2, bad(np.nan)), STATE), ((0, 1, 16385, 1, one), ARG), ((model, 0, 16385, 0, one), ARG),
    ]
    for (m, i, w, h, rgb), code in refusals:
        assert L.pt_set_lightmap(r.ctx, m, i, w, h, _p(rgb)) == code, (m, i, w, h, code)
        assert r.lightmap_info(model, 0) == (5, 3)
    w = C.c_uint32(7); h = C.c_uint32(7)
    assert L.pt_get_lightmap_info(r.ctx, -1, 0, C.byref(w), C.byref(h)) == ARG
    assert L.pt_get_lightmap_info(r.ctx, model, 1, C.byref(w), C.byref(h)) == ARG
    assert L.pt_get_lightmap_info(r.ctx, model, 0, None, C.byref(h)) == ARG
    assert (w.value, h.value) == (7, 7)
    after = r.lightmap_lookup(inst, prim, u, v)
    assert_bit_equal(after[0], before[0], "lookup after refused calls")
    assert before[1].all() and after[1].all() and _info(r) == info
    # setting and clearing move neither the build nor the flattened scene
    r.set_lightmap(model, 0, small)
    assert r.lightmap_info(model, 0) == (2, 2) and _info(r) == info
    r.set_lightmap(model, 0, None)
    assert r.lightmap_info(model, 0) == (0, 0) and _info(r) == info
    r.set_lightmap(model, 0, None)                                                 # clearing what is not there is fine
    got = r.lightmap_lookup(inst, prim, u, v)
    assert not got[0].any() and not got[1].any()
    # the division is the wrapper's
    r.set_lightmap_sums(model, 0, good * F(8.0), 8)
    assert_bit_equal(r.lightmap_lookup(inst, prim, u, v)[0], before[0], "sums / n")
    with pytest.raises(api.PtError):
        r.set_lightmap_sums(model, 0, good, 0)


def test_the_limit_on_all_maps_together(api):
    """2^28 texels in all: a 16384 x 16384 map fills it, so one more texel anywhere is refused.  The big map is never set (it would take
    4 GiB): the limit is met by sides alone, which are checked before a texel is read"""
    sc, model = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)
    r.set_lightmap(model, 0, np.ones((1, 1, 3), F))
    other = [i for i, m in enumerate(sc.models) if m.name == "cb_box_tall"][0]
    r.set_model_uvs(other, LC.box_atlas(sc.models[other].positions))
    r.rebuild()
    one = np.zeros(3, F)
    assert r.L.pt_set_lightmap(r.ctx, other, 0, 16384, 16384, _p(one)) == LIMIT     # 2^28 + the texel already there
    assert r.lightmap_info(other, 0) == (0, 0) and r.lightmap_info(model, 0) == (1, 1)


def test_baked_refusals_come_before_any_device_call(api):
    L = api.lib()
    cfg = api.Config(48, 32, 8, 512, 1, LC.SEED, 0, 1, 4, 0, -1, 0, 0, 0, 0, 0)
    ctx = C.c_void_p(L.pt_create(C.byref(cfg)))
    try:
        prm = api.BakedParams(0)
        assert L.pt_render_baked(ctx, 0, 1, C.byref(prm), None) == STATE            # not built
        assert L.pt_lightmap_lookup(ctx, 0, 1, None, None, None, None, None, None) == STATE
        assert L.pt_read_baked(ctx, None) == STATE
        assert L.pt_write_baked_image(ctx, b"never.png") == STATE
        assert L.pt_reset_baked(ctx) == 0
    finally:
        L.pt_destroy(ctx)
    r = api.Renderer(LC.quad_scene(), 48, 32)                                      # built, but no camera
    assert L.pt_render_baked(r.ctx, 0, 1, C.byref(api.BakedParams(0)), None) == STATE
    assert "camera" in L.pt_last_error(r.ctx).decode()
    sc, _ = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)

    def prm(hops=0, unlit=(0.0, 0.0, 0.0), word=None):
        p = api.BakedParams(hops, (C.c_float * 3)(*unlit))
        if word is not None:
            p.reserved[word] = 1
        return p
    cases = [(0, 1, prm(9)), (0, 0, prm()), (0xFFFFFFFE, 3, prm()), (0, 1, prm(unlit=(-1.0, 0, 0))), (0, 1, prm(unlit=(0, np.nan, 0))),
             (0, 1, prm(unlit=(0, 0, np.inf)))] + [(0, 1, prm(word=k)) for k in range(4)]
    for first, n, p in cases:
        assert L.pt_render_baked(r.ctx, first, n, C.byref(p), None) == ARG, (first, n, p.max_hops, list(p.unlit), list(p.reserved))
    assert L.pt_render_baked(r.ctx, 0, 1, None, None) == ARG
    assert L.pt_read_baked(r.ctx, None) == STATE                                   # nothing was rendered by the refused calls
    # the lookup's own refusals
    q = np.zeros(1, np.uint32); f = np.zeros(1, F); out = np.zeros(3, F); m = np.zeros(1, np.uint8)
    n_leaves = sum(mod.matrices.shape[0] for mod in sc.models)
    for inst, prim in ((n_leaves, 0), (0, 10 ** 6)):
        assert L.pt_lightmap_lookup(r.ctx, 0, 1, _p(np.array([inst], np.uint32)), _p(np.array([prim], np.uint32)), _p(f), _p(f), _p(out), _p(m)) == ARG
    assert L.pt_lightmap_lookup(r.ctx, 0, 1, _p(q), _p(q), _p(f), _p(f), None, _p(m)) == ARG
    assert L.pt_lightmap_lookup(r.ctx, 0, 0, None, None, None, None, None, None) == 0


def test_host_lookup_is_the_definition(api):
    sc, maps = BC.soup_scene()
    r = api.Renderer(sc, 48, 32)
    BC.set_maps(r, maps)
    inst, prim, u, v = BC.soup_queries(sc)
    want, want_mapped = BC.scene_lookup(sc, maps, inst, prim, u, v)
    got, mapped = r.lightmap_lookup(inst, prim, u, v)
    assert_bit_equal(got, want, "host lookup on the soup")
    assert np.array_equal(mapped, want_mapped)
    # leaves 1 and 2 (ordinals 0, 1 of the soup) are mapped, leaf 0 (no UVs) and leaf 3 (ordinal 2) are not
    assert np.array_equal(mapped, np.isin(inst, (1, 2)).astype(np.uint8)) and mapped.any() and not mapped.all()
    assert not got[mapped == 0].any()
    # the same hits on the two mapped instances see different maps
    a = r.lightmap_lookup(np.full(50, 1, np.uint32), prim[:50] % 40, u[:50], v[:50])[0]
    b = r.lightmap_lookup(np.full(50, 2, np.uint32), prim[:50] % 40, u[:50], v[:50])[0]
    assert not np.array_equal(a, b)


def test_the_clamp_on_every_side_and_corner(api):
    sc = BC.clamp_scene()
    r = api.Renderer(sc, 48, 32)
    tex = np.random.default_rng(3).uniform(0.0, 1.0, (3, 5, 3)).astype(F)
    r.set_lightmap(0, 0, tex)
    k = len(BC.CLAMP_UVS)
    inst, prim = np.zeros(k, np.uint32), np.arange(k, dtype=np.uint32)
    u, v = np.full(k, 0.3, F), np.full(k, 0.2, F)
    got, mapped = r.lightmap_lookup(inst, prim, u, v)
    assert mapped.all()
    assert_bit_equal(got, BC.lookup(tex, sc.models[0].uvs, u, v), "clamped lookups")
    # the four corners are texels themselves, whatever lies beyond: (s, t) far out on both axes
    corner = {4: tex[0, 0], 5: tex[0, 4], 6: tex[2, 0], 7: tex[2, 4], 8: tex[2, 0]}
    for q, texel in corner.items():
        assert_bit_equal(got[q], texel, f"corner query {q}")
    # ... and the four sides clamp one coordinate only: the value is constant along the outward axis
    for q, (s, t) in enumerate(BC.CLAMP_UVS[:4]):
        far = np.array([[[10 * s, t] if abs(s) > 1 else [s, 10 * t]] * 3], F)
        assert_bit_equal(BC.lookup(tex, far, u[:1], v[:1])[0], got[q], f"side query {q}")


@pytest.mark.parametrize("size", [(8, 8), (16, 16), (16, 4)])
def test_texel_centres_are_exact_on_power_of_two_maps(api, size):
    w, h = size
    sc = BC.centre_scene(w, h)
    r = api.Renderer(sc, 48, 32)
    tex = np.random.default_rng(4).uniform(0.0, 1.0, (h, w, 3)).astype(F)
    r.set_lightmap(0, 0, tex)
    n = w * h
    rng = np.random.default_rng(5)
    u = rng.uniform(0, 1, n).astype(F)
    v = (rng.uniform(0, 1, n) * (1 - u)).astype(F)
    got, mapped = r.lightmap_lookup(np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), u, v)
    assert mapped.all()
    assert_bit_equal(got.reshape(h, w, 3), tex, "texel centres through collapsed UVs")


def test_round_trip_with_the_bakes_convention(api):
    """every covered texel of the bake's own texel table, looked up at its own (prim, u, v), is that texel to within 1e-3: the UV
    interpolation is a few ulps of s off, times w = 16, times a texel difference of at most 1, about 1e-5; a half-texel slip shows as
    differences of order 0.3"""
    sc, model = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)
    w = h = 16
    tex = np.random.default_rng(6).uniform(0.0, 1.0, (h, w, 3)).astype(F)
    r.set_lightmap(model, 0, tex)
    prim, uv, _, _ = r.lightmap_texels(model, 0, w, h)
    cov = prim != LC.MISS
    assert cov.sum() == 193
    leaf = [k for k, (m, _) in enumerate(BC.leaf_keys(sc)) if m == model][0]
    got, mapped = r.lightmap_lookup(np.full(cov.sum(), leaf, np.uint32), prim[cov], uv[cov][:, 0], uv[cov][:, 1])
    assert mapped.all()
    err = np.abs(got.astype(np.float64) - tex[cov])
    print(f"round trip over {int(cov.sum())} covered texels: max abs error {err.max():.3g}")
    assert err.max() < 1e-3
    # what the bound is there to catch
    shifted = BC.lookup(tex, sc.models[model].uvs[prim[cov]] + F(0.5 / w), uv[cov][:, 0], uv[cov][:, 1])
    assert np.abs(shifted.astype(np.float64) - tex[cov]).max() > 0.1


def test_lifetime_of_the_maps(api):
    sc, maps = BC.soup_scene()
    r = api.Renderer(sc, 48, 32)
    BC.set_maps(r, maps)
    third = np.full((2, 2, 3), 0.5, F)
    r.set_lightmap(1, 2, third)
    mats = sc.models[1].matrices
    r.rebuild()                                                                    # pt_build keeps them
    assert [r.lightmap_info(1, k) for k in range(3)] == [(5, 3), (8, 8), (2, 2)]
    # fewer instances: the ordinals that still exist keep their maps
    r.set_instances(1, mats[:2])
    r.rebuild()
    assert [r.lightmap_info(1, k) for k in range(2)] == [(5, 3), (8, 8)]
    assert r.L.pt_get_lightmap_info(r.ctx, 1, 2, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == ARG
    inst, prim, u, v = BC.soup_queries(sc)
    keep = inst < 3
    got, mapped = r.lightmap_lookup(inst[keep], prim[keep], u[keep], v[keep])
    want, want_mapped = BC.scene_lookup(sc, maps, inst[keep], prim[keep], u[keep], v[keep])
    assert_bit_equal(got, want, "after dropping an instance")
    assert np.array_equal(mapped, want_mapped)
    # more instances again: the dropped ordinal comes back without its map, a moved one keeps its (now stale) lighting
    moved = mats.copy()
    moved[0] = mats[2]
    r.set_instances(1, moved)
    r.rebuild()
    assert [r.lightmap_info(1, k) for k in range(3)] == [(5, 3), (8, 8), (0, 0)]
    got, mapped = r.lightmap_lookup(inst, prim, u, v)
    want, want_mapped = BC.scene_lookup(sc, maps, inst, prim, u, v)
    assert_bit_equal(got, want, "after moving and re-adding instances")
    assert np.array_equal(mapped, want_mapped)
    # new UVs on the model drop its maps; the other models' stay
    sc2, model = LC.cornell_atlas_scene()
    q = api.Renderer(sc2, 48, 32)
    other = [i for i, m in enumerate(sc2.models) if m.name == "cb_box_tall"][0]
    q.set_model_uvs(other, LC.box_atlas(sc2.models[other].positions))
    q.rebuild()
    q.set_lightmap(model, 0, third)
    q.set_lightmap(other, 0, third)
    q.set_model_uvs(other, LC.box_atlas(sc2.models[other].positions))
    q.rebuild()
    assert q.lightmap_info(other, 0) == (0, 0) and q.lightmap_info(model, 0) == (2, 2)
