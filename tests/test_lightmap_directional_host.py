"""CPU: directional lightmaps (pt_bake_lightmap_directional, pt_lightmap_gradient, pt_set_lightmap_directional,
pt_get_lightmap_directional_info, pt_lightmap_lookup_directional) without a GPU: the symbols, every refusal with "nothing changed" checked,
the host gradient and the host lookup against the numpy restatements of tests/lightmap_directional_common.py bit for bit, the algebra the
gradient rests on, delta = 0, the clamp, and the gradients' lifetime.  (The fold, the device side and the view: tests/test_gpu_lightmap_directional.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import baked_common as BC
import lightmap_common as LC
import lightmap_directional_common as DC
import normalmap_common as NM
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, STATE, LIMIT = -1, -3, -5
NEW_SYMBOLS = ["pt_bake_lightmap_directional", "pt_lightmap_gradient", "pt_set_lightmap_directional", "pt_get_lightmap_directional_info",
               "pt_lightmap_lookup_directional"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_the_five_exports_exist(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    for method in ("bake_lightmap_directional", "lightmap_gradient", "dilate_lightmap_directional", "set_lightmap_directional", "lightmap_directional_info",
                   "lightmap_lookup_directional"):
        assert callable(getattr(api.Renderer, method))
    assert "directional maps" not in header                                      # off the out-of-scope lists


def _queries(model, n=6):
    return np.zeros(n, np.uint32) + model, np.arange(n, dtype=np.uint32), np.full(n, 0.25, F), np.full(n, 0.5, F)


def test_set_directional_refusals_change_nothing(api):
    sc, model = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)
    rng = np.random.default_rng(1)
    tex = rng.uniform(0, 1, (3, 5, 3)).astype(F)
    good = rng.uniform(-1, 1, (3, 5, 3, 3)).astype(F)
    other = [i for i, m in enumerate(sc.models) if m.name == "cb_box_tall"][0]       # a placement without a map
    L = r.L
    assert L.pt_set_lightmap_directional(r.ctx, model, 0, 5, 3, _p(good)) == STATE    # no scalar map yet
    r.set_lightmap(model, 0, tex)
    assert not r.lightmap_directional_info(model, 0)
    r.set_lightmap_directional(model, 0, good)
    assert r.lightmap_directional_info(model, 0)
    q = _queries(model)
    d = np.tile(np.array([0.3, -0.8, 0.5], F), (len(q[0]), 1))
    before = (r.lightmap_lookup(*q), r.lightmap_lookup_directional(*q, d), r.scene_info().as_dict())

    def bad(value):
        a = good.copy()
        a[2, 1, 0, 2] = value
        return a
    refusals = [((-1, 0, 5, 3, good), ARG), ((len(sc.models), 0, 5, 3, good), ARG), ((model, 1, 5, 3, good), ARG),
                ((model, 0, 0, 3, good), ARG), ((model, 0, 5, 0, good), ARG), ((model, 0, 5, 3, None), ARG), ((model, 0, 0, 3, None), ARG),
                ((model, 0, 3, 5, good), ARG), ((model, 0, 5, 4, good), ARG),            # not the map's size
                ((model, 0, 5, 3, bad(np.nan)), ARG), ((model, 0, 5, 3, bad(np.inf)), ARG), ((model, 0, 5, 3, bad(-np.inf)), ARG),
                ((other, 0, 5, 3, good), STATE), ((other, 0, 5, 3, bad(np.nan)), STATE), ((0, 0, 5, 3, good), STATE)]
    for (m, i, w, h, g), code in refusals:
        assert L.pt_set_lightmap_directional(r.ctx, m, i, w, h, _p(g)) == code, (m, i, w, h, code)
        assert r.lightmap_info(model, 0) == (5, 3) and r.lightmap_directional_info(model, 0)
    has = C.c_uint32(7)
    assert L.pt_get_lightmap_directional_info(r.ctx, -1, 0, C.byref(has)) == ARG
    assert L.pt_get_lightmap_directional_info(r.ctx, model, 1, C.byref(has)) == ARG
    assert L.pt_get_lightmap_directional_info(r.ctx, model, 0, None) == ARG and has.value == 7
    assert_bit_equal(r.lightmap_lookup(*q)[0], before[0][0], "scalar lookup after refused calls")
    assert_bit_equal(r.lightmap_lookup_directional(*q, d)[0], before[1][0], "directional lookup after refused calls")
    assert r.scene_info().as_dict() == before[2]
    # a negative value is legal, clearing what is not there is fine, and neither moves the build
    r.set_lightmap_directional(model, 0, -np.abs(good))
    r.set_lightmap_directional(other, 0, None)
    r.set_lightmap_directional(model, 0, None)
    r.set_lightmap_directional(model, 0, None)
    assert not r.lightmap_directional_info(model, 0) and r.lightmap_info(model, 0) == (5, 3) and r.scene_info().as_dict() == before[2]


def test_bake_and_gradient_refusals_come_before_any_device_call(api):
    sc, model = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)
    L = r.L
    sums, dirs, cov = np.full((2, 2, 3), 5, F), np.full((2, 2, 3, 3), 7, F), np.zeros((2, 2), np.uint8)

    def bake(m=model, i=0, w=2, h=2, n=4, s=sums, d=dirs, **kw):
        prm = api.LightmapParams(m, i, w, h, kw.get("first", 0), n, kw.get("key_base", 0), kw.get("bias", 0.0))
        return L.pt_bake_lightmap_directional(r.ctx, C.byref(prm), _p(s), _p(d), _p(cov))
    assert bake(d=None) == ARG and bake(s=None) == ARG and bake(m=-1) == ARG and bake(i=3) == ARG and bake(w=0) == ARG and bake(n=0) == ARG
    assert bake(bias=float("nan")) == ARG and bake(key_base=0xFFFFFFFF) == ARG and bake(first=0xFFFFFFFF, n=2) == ARG
    assert bake(m=0) == STATE and bake(w=16385, h=1) == LIMIT
    assert L.pt_bake_lightmap_directional(r.ctx, None, _p(sums), _p(dirs), _p(cov)) == ARG
    assert (sums == 5).all() and (dirs == 7).all() and not cov.any()
    grad = np.full((2, 2, 3, 3), 9, F)
    g = lambda m=model, i=0, w=2, h=2, n=4, a=dirs, b=grad: L.pt_lightmap_gradient(r.ctx, 0, m, i, w, h, n, _p(a), _p(b))
    assert g(a=None) == ARG and g(b=None) == ARG and g(m=-1) == ARG and g(i=1) == ARG and g(w=0) == ARG and g(n=0) == ARG and g(m=0) == STATE
    assert g(w=16385, h=1) == LIMIT and (grad == 9).all()
    assert r.stats().paths == 0


def test_host_gradient_is_the_restatement(api):
    """a random-UV soup under a general rigid placement: the table's normals are interpolated, turned and not renormalised"""
    sc = DC.sparse_soup()
    r = api.Renderer(sc, 48, 32)
    m = sc.models[0]
    w, h, n = 9, 7, 13
    for inst in (0, 1):
        table = LC.texels(m.positions, m.normals, m.uvs, m.matrices[inst], w, h)
        cov = table[0] != LC.MISS
        assert 5 < cov.sum() < w * h
        dirs = np.random.default_rng(5 + inst).uniform(-3, 3, (h, w, 3, 3)).astype(F)
        got = r.lightmap_gradient(0, inst, dirs, n)
        assert_bit_equal(got, DC.gradient(dirs, table[3], cov, n), f"instance {inst}")
        assert not got[~cov].any() and np.abs(got[cov]).min() > 0


def test_the_algebra_of_the_gradient(api):
    """L = a + b.d over the hemisphere about n gives M0 = a + (2/3) b.n and M1 = (2/3) a n + b/4 + (b.n) n/4 (float64 here); the gradient of
    n_samples * M1 must be (2/3)(b - (b.n) n) within 1e-4 of |a| + |b|: binary32 inputs and constants round at 6e-8, the table's normal is a
    unit vector to a few 1e-7, and the expression amplifies by less than 10"""
    sc = DC.sparse_soup()
    r = api.Renderer(sc, 48, 32)
    w, h, n_samples = 9, 7, 64
    prim, _, _, normal = r.lightmap_texels(0, 1, w, h)
    cov = prim != LC.MISS
    rng = np.random.default_rng(17)
    a = rng.uniform(0.0, 2.0, (h, w, 3))                                           # per channel
    b = rng.normal(size=(h, w, 3, 3))                                              # [axis][channel]
    n = normal.astype(np.float64)
    bn = (b * n[..., :, None]).sum(axis=2)                                         # b.n per channel
    m1 = (2.0 / 3.0) * a[..., None, :] * n[..., :, None] + b / 4.0 + bn[..., None, :] * n[..., :, None] / 4.0
    got = r.lightmap_gradient(0, 1, (m1 * n_samples).astype(F), n_samples).astype(np.float64)
    want = (2.0 / 3.0) * (b - bn[..., None, :] * n[..., :, None])
    scale = np.abs(a).max(axis=-1) + np.sqrt((b * b).sum(axis=2)).max(axis=-1)
    err = (np.abs(got - want).max(axis=(2, 3)) / scale)[cov]
    print("gradient algebra: largest relative error", err.max())
    assert cov.sum() > 10 and err.max() < 1e-4


def _hook(api):
    sc = NM.hook_scene()
    r = api.Renderer(sc, 48, 32)
    maps, grads = DC.hook_maps(sc)
    DC.set_all(r, maps, grads)
    return sc, r, maps, grads


def test_host_lookup_is_the_restatement(api):
    sc, r, maps, grads = _hook(api)
    inst, prim, u, v, d = NM.hook_queries(sc, 1500)
    delta, _, _, _ = DC.deltas(sc, r.tlas_instances(0), inst, prim, u, v, d)
    want, want_mapped = DC.scene_lookup_dir(sc, maps, grads, inst, prim, u, v, delta)
    got, mapped = r.lightmap_lookup_directional(inst, prim, u, v, d)
    assert np.array_equal(mapped, want_mapped) and mapped.any() and not mapped.all()
    assert_bit_equal(got, want, "host directional lookup")
    keys = BC.leaf_keys(sc)
    with_grad = np.array([keys[i] in grads for i in inst])
    moved = np.abs(delta).max(axis=1) > 0
    scalar = r.lightmap_lookup(inst, prim, u, v)[0]
    assert (with_grad & moved).sum() > 100 and not np.array_equal(got[with_grad & moved], scalar[with_grad & moved])
    assert_bit_equal(got[~with_grad], scalar[~with_grad], "a map without a gradient is looked up as before")


def test_delta_zero_returns_the_scalar_lookup(api):
    """flat normal maps (delta = n - n) and materials without one (delta = 0 by construction) under random finite gradients"""
    sc = NM.hook_scene(flat=True)
    r = api.Renderer(sc, 48, 32)
    maps, _ = DC.hook_maps(sc)
    rng = np.random.default_rng(41)
    grads = {key: (rng.uniform(-1, 1, tex.shape[:2] + (3, 3)) * 10.0 ** rng.integers(-30, 30, tex.shape[:2] + (3, 3))).astype(F) for key, tex in maps.items()}
    DC.set_all(r, maps, grads)
    inst, prim, u, v, d = NM.hook_queries(sc, 1500)
    got, mapped = r.lightmap_lookup_directional(inst, prim, u, v, d)
    want, want_mapped = r.lightmap_lookup(inst, prim, u, v)
    assert np.array_equal(mapped, want_mapped) and mapped.sum() > 500
    assert_bit_equal(got, want, "delta = 0")


def test_the_clamp_never_returns_a_negative_or_a_nan(api):
    sc, r, maps, _ = _hook(api)
    rng = np.random.default_rng(43)
    big = np.finfo(F).max
    hostile = {key: rng.choice(np.array([-big, big, -1e30, 1e30, -1.0, 0.0, 1e-40], F), tex.shape[:2] + (3, 3)) for key, tex in maps.items()}
    for key in maps:
        maps[key] = rng.choice(np.array([0.0, 1e-40, 1.0, big], F), maps[key].shape)
    DC.set_all(r, maps, hostile)
    inst, prim, u, v, d = NM.hook_queries(sc, 3000)
    with np.errstate(all="ignore"):
        got, mapped = r.lightmap_lookup_directional(inst, prim, u, v, d)
        delta, _, _, _ = DC.deltas(sc, r.tlas_instances(0), inst, prim, u, v, d)
        want, _ = DC.scene_lookup_dir(sc, maps, hostile, inst, prim, u, v, delta)
    assert not np.isnan(got).any() and (got >= 0).all() and (got[mapped == 1] > 0).any() and (got[mapped == 1] == 0).any()
    assert_bit_equal(got, want, "hostile gradients")


def test_the_gradient_lives_and_dies_with_its_map(api):
    sc, maps = BC.soup_scene()
    r = api.Renderer(sc, 48, 32)
    grads = DC.soup_grads(maps)
    DC.set_all(r, maps, grads)
    has = lambda: [r.lightmap_directional_info(1, k) for k in range(len(r_matrices))]
    r_matrices = list(sc.models[1].matrices)
    assert has() == [True, True, False]
    r.rebuild()                                                                    # pt_build keeps it
    assert has() == [True, True, False]
    r.set_lightmap(1, 0, maps[1, 0])                                               # a new map drops the old gradient
    assert has() == [False, True, False] and r.lightmap_info(1, 0) == (5, 3)
    r.set_lightmap(1, 1, None)                                                     # ... and so does clearing the map
    assert has() == [False, False, False]
    r.set_lightmap(1, 1, maps[1, 1])
    assert has() == [False, False, False]                                          # it does not come back with a new map
    r.set_lightmap_directional(1, 1, grads[1, 1])
    r.set_instances(1, np.stack(r_matrices[:2]))                                    # the ordinals that still exist keep theirs
    r.rebuild()
    r_matrices = r_matrices[:2]
    assert has() == [False, True] and r.lightmap_info(1, 1) == (8, 8)
    r.set_instances(1, np.stack(r_matrices[:1]))
    r.rebuild()
    r_matrices = r_matrices[:1]
    assert has() == [False]
    r.set_lightmap_directional(1, 0, grads[1, 0])
    assert has() == [True]
    r.set_model_uvs(1, sc.models[1].uvs)                                           # new UVs drop the maps, and the gradients with them
    r.rebuild()
    assert has() == [False] and r.lightmap_info(1, 0) == (0, 0)
