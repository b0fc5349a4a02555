"""CPU: lightmaps (pt_bake_lightmap, pt_lightmap_texels, pt_lightmap_ray, pt_lightmap_dilate) without a GPU: the symbols, every refusal that
include/pt_api.h promises before any device call, the host evaluation of the texel table and of the sample directions against the numpy
restatement of tests/lightmap_common.py.  No GPU is touched (dilation and the bake itself run on the device: tests/test_gpu_lightmap.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import lightmap_common as LC
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, STATE, LIMIT = -1, -3, -5
NEW_SYMBOLS = ["pt_bake_lightmap", "pt_lightmap_texels", "pt_lightmap_ray", "pt_lightmap_dilate"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


@pytest.fixture(scope="module")
def cornell(api):
    sc, model = LC.cornell_atlas_scene()
    return api.Renderer(sc, 48, 32), model


def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert "typedef struct pt_lightmap_params" in header
    for method in ("bake_lightmap", "lightmap_texels", "lightmap_ray", "dilate_lightmap"):
        assert callable(getattr(api.Renderer, method))
    assert C.sizeof(api.LightmapParams) == 48
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    assert "bake_lightmap(" in wrapper and "dilate_lightmap(" in wrapper


def _bake(r, prm, sums, cov):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return r.L.pt_bake_lightmap(r.ctx, None if prm is None else C.byref(prm), p(sums), p(cov))


def test_bake_arguments_are_refused_and_nothing_changes(api, cornell):
    r, model = cornell
    w, h = 12, 8
    start = np.random.default_rng(1).uniform(0, 1, (h, w, 3)).astype(F)
    sums = start.copy(); cov = np.full((h, w), 7, np.uint8)

    def prm(**kw):
        v = dict(model=model, instance=0, w=w, h=h, first_sample=0, n_samples=4, key_base=0, bias=0.25)
        v.update(kw)
        return api.LightmapParams(v["model"], v["instance"], v["w"], v["h"], v["first_sample"], v["n_samples"], v["key_base"], v["bias"])

    big = np.zeros(1, F)          # never read: each of these is refused for its sizes alone
    refusals = [
        (prm(model=-1), ARG), (prm(model=6), ARG), (prm(instance=1), ARG), (prm(w=0), ARG), (prm(h=0), ARG), (prm(n_samples=0), ARG),
        (prm(bias=np.nan), ARG), (prm(bias=np.inf), ARG), (prm(bias=-np.inf), ARG),
        (prm(key_base=0xFFFFFFFF - w * h + 2), ARG), (prm(first_sample=0xFFFFFFFE, n_samples=3), ARG),
        (prm(model=0), STATE),                                                   # cb_light carries no UVs
        (prm(w=16385, h=1), LIMIT), (prm(w=1, h=16385), LIMIT), (prm(w=16384, h=8192), LIMIT),
    ]
    for p, code in refusals:
        target = big if (p.w, p.h) != (w, h) else sums
        assert _bake(r, p, target, cov) == code, (p.model, p.instance, p.w, p.h, p.n_samples, p.key_base, p.first_sample, p.bias, code)
    for word in range(4):
        bad = prm()
        bad.reserved[word] = 1
        assert _bake(r, bad, sums, cov) == ARG
    assert _bake(r, None, sums, cov) == ARG
    assert _bake(r, prm(), None, cov) == ARG
    # the largest key and the last sample themselves are fine arguments: refused only later, for the next reason in line
    assert _bake(r, prm(key_base=0xFFFFFFFF - w * h + 1, first_sample=0xFFFFFFFD, n_samples=3, bias=np.nan), sums, cov) == ARG
    assert "bias" in r.L.pt_last_error(r.ctx).decode()
    assert_bit_equal(sums, start, "sums after refused calls")
    assert (cov == 7).all()
    with pytest.raises(api.PtError) as e:
        r.bake_lightmap(model, 3, w, h, 4)
    assert e.value.code == ARG


def test_bake_needs_a_built_scene_and_a_light_for_nee(api):
    L = api.lib()
    cfg = api.Config(48, 32, 8, 512, 1, LC.SEED, 0, 1, 4, 0, -1, 0, 0, 0, 0, 0)
    ctx = C.c_void_p(L.pt_create(C.byref(cfg)))
    sums = np.zeros((4, 4, 3), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        prm = api.LightmapParams(0, 0, 4, 4, 0, 1, 0, 0.0)
        assert L.pt_bake_lightmap(ctx, C.byref(prm), p(sums), None) == STATE
        assert L.pt_lightmap_texels(ctx, 0, 0, 4, 4, 0, None, None, None, None) == STATE
    finally:
        L.pt_destroy(ctx)
    # NEE is on by default and the quad scene has no emissive model: the bake is refused, the texel table (which integrates nothing) is not
    r = api.Renderer(LC.quad_scene(), 48, 32)
    prm = api.LightmapParams(0, 0, 4, 4, 0, 1, 0, 0.0)
    assert L.pt_bake_lightmap(r.ctx, C.byref(prm), p(sums), None) == STATE
    assert "emissive" in L.pt_last_error(r.ctx).decode()
    assert (r.lightmap_texels(0, 0, 4, 4)[0] != LC.MISS).all()
    assert not sums.any()


def test_texel_and_dilate_arguments_are_refused(api, cornell):
    r, model = cornell
    L = r.L
    for args, code in (((-1, 0, 4, 4), ARG), ((6, 0, 4, 4), ARG), ((model, 1, 4, 4), ARG), ((model, 0, 0, 4), ARG), ((model, 0, 4, 0), ARG),
                       ((0, 0, 4, 4), STATE), ((model, 0, 16385, 1), LIMIT), ((model, 0, 8193, 8192), LIMIT)):
        for on_device in (0, 1):
            assert L.pt_lightmap_texels(r.ctx, *args, on_device, None, None, None, None) == code, (args, on_device)
    rgb = np.ones((4, 4, 3), F); cov = np.zeros((4, 4), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    assert L.pt_lightmap_dilate(r.ctx, 4, 4, 1, None, p(cov)) == ARG
    assert L.pt_lightmap_dilate(r.ctx, 4, 4, 1, p(rgb), None) == ARG
    assert L.pt_lightmap_dilate(r.ctx, 0, 4, 1, p(rgb), p(cov)) == ARG
    assert L.pt_lightmap_dilate(r.ctx, 4, 0, 1, p(rgb), p(cov)) == ARG
    assert L.pt_lightmap_dilate(r.ctx, 16385, 1, 1, p(rgb), p(cov)) == LIMIT
    assert L.pt_lightmap_dilate(r.ctx, 16384, 8192, 1, p(rgb), p(cov)) == LIMIT
    assert L.pt_lightmap_dilate(r.ctx, 4, 4, 0, p(rgb), p(cov)) == 0            # no pass: nothing to do, no device
    assert (rgb == 1).all() and not cov.any()
    assert L.pt_lightmap_ray(r.ctx, 0, 0, None, p(rgb)) == ARG
    assert L.pt_lightmap_ray(r.ctx, 0, 0, p(rgb), None) == ARG


@pytest.mark.parametrize("name", LC.TEXEL_CASES)
def test_host_texel_table_is_the_definition(api, name):
    case = LC.texel_case(name)
    want = LC.expected_texels(case)
    LC.check_case_is_meaningful(name, want)
    got = LC.query_texels(api, case, on_device=False)
    assert np.array_equal(got[0], want[0]), f"{name}: owners"
    for g, w, what in zip(got[1:], want[1:], ("uv", "position", "normal")):
        assert_bit_equal(g, w, f"{name}: {what}")


def test_edge_centres_of_the_16x16_box_map():
    """38 centres of the 16 x 16 box map lie exactly on an edge of their triangle: the case is there for the shared-edge rule"""
    for box in ("cb_box_short", "cb_box_tall"):
        sc, model = LC.cornell_atlas_scene(box)
        assert LC.on_an_edge(sc.models[model].uvs, 16, 16) == 38


def _normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v = (v / np.sqrt((v * v).sum(1, keepdims=True))).astype(F)
    v[:6] = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0.6, 0.8, 0.0], [0.6, 0.0, -0.8]], F)
    return v


def test_lightmap_ray_is_the_definition(api, oracle_mod, cornell):
    """4 096 (key, sample, normal) triples, keys up to 2^32 - 1, samples beyond n_sobol = 512, normals all over the sphere"""
    r, _ = cornell
    rng = np.random.default_rng(6)
    keys = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
    keys[:4] = (0, 1, 0x80000000, 0xFFFFFFFF)
    samples = rng.integers(0, 4000, 4096, dtype=np.uint64)
    samples[:4] = (0, 511, 512, 0xFFFFFFFF)
    normals = _normals(4096, 7)
    assert (normals[:, 2] < 0).sum() > 1000
    want = LC.rays(oracle_mod, keys, samples, normals)
    got = np.array([r.lightmap_ray(int(k), int(s), n) for k, s, n in zip(keys, samples, normals)], F)
    assert_bit_equal(got, want, "lightmap directions")


def test_directions_follow_the_cosine_law(api, cornell):
    """Guards against a convention error shared by code and restatement.  4 096 samples of one key: unit directions on the normal's side whose
    mean cosine is 2/3: cos theta under the cosine law has standard deviation 0.236, so 0.01 is 2.7 sigma / sqrt(4096) for random points, and
    Sobol points do better."""
    r, _ = cornell
    for n in (np.array([0, 0, 1], F), np.array([0.6, 0.0, -0.8], F), _normals(8, 3)[7]):
        d = np.array([r.lightmap_ray(77, s, n) for s in range(4096)], np.float64)
        assert np.abs(np.sqrt((d * d).sum(1)) - 1.0).max() < 1e-6
        cos = d @ n.astype(np.float64)
        assert (cos > 0).all(), cos.min()
        assert abs(cos.mean() - 2.0 / 3.0) < 0.01, cos.mean()
