"""CPU: lightmap bakes with direct light sampled at the texel, without a GPU: the symbols; every refusal include/pt_api.h promises before any
device call, in its order; the light sample evaluated on the host (pt_lightmap_light_sample with on_device = 0) bit for bit against the
numpy restatement of tests/lightmap_direct_common.py; and two checks of the DEFINITION that are independent of the library: the direct term
against Lambert's closed form for the irradiance of a polygon, and the whole sample's mean against the plain gather's.  No GPU is touched
(the kernels and the bakes: tests/test_gpu_lightmap_direct.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import lightmap_common as LC
import lightmap_direct_common as LD
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, HIP, STATE, LIMIT = -1, -2, -3, -5
SIGMAS = 5.0          # tests/irradiance_closed_common.py's pass rule: standard errors of the samples' own spread


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- 1. exports
def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in ("pt_bake_lightmap_direct", "pt_bake_lightmap_adaptive_direct", "pt_lightmap_light_sample"):
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert C.sizeof(api.LightmapDirect) == 16 and "} pt_lightmap_direct;" in header
    for method in ("bake_lightmap_direct", "bake_lightmap_adaptive_direct", "lightmap_light_sample"):
        assert callable(getattr(api.Renderer, method))
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for name in ("bake_lightmap_direct(", "bake_lightmap_adaptive_direct("):
        assert name in wrapper, name
    # the item left the plain bake's out-of-scope list, and the new section states its own
    assert "conservative or supersampled coverage, direct light sampled at the texel" not in header
    assert "MIS between the texel's light sample and its gather ray" in header


# ---- 2. refusals
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _many_models(lamp_at):
    """258 one-triangle models, model 0 with UVs; model `lamp_at` is the lamp"""
    from path_tracer_amd.scene_desc import Emissive, Lambertian, Model, SceneDesc
    grey = Lambertian.new((0.5, 0.5, 0.5))
    models = []
    for i in range(258):
        p = (LC.QUAD_POS[:1] + np.array([0, 0, 0.01 * i], F)).astype(F)
        if i == lamp_at:
            models.append(Model.new(p + np.array([0, 0, 5], F), -LC.QUAD_NRM[:1], Emissive.new((5.0, 5.0, 5.0)), None, "lamp", uvs=LC.QUAD_UV[:1] if i == 0 else None))
        else:
            models.append(Model.new(p, LC.QUAD_NRM[:1], grey, None, f"m{i}", uvs=LC.QUAD_UV[:1] if i == 0 else None))
    return SceneDesc.new(models, None, "258 models")


def _media_scene():
    """quad_scene(light=True) with a glass block that carries a volume"""
    from path_tracer_amd.scene_desc import Dielectric, Model, Volume
    from textures_common import box
    sc = LC.quad_scene(light=True)
    bp, bn = box((0.2, 0.2, 0.5), (0.6, 0.6, 0.9))
    sc.models.append(Model.new(bp, bn, Dielectric.new((1.0, 1.0, 1.0), 1.5, Volume.new((0.1, 0.2, 0.3), 1.0, 0.5, 0.0)), None, "fog"))
    return sc


def test_refusals_fire_in_order_before_any_device_call_and_nothing_changes(api):
    w, h, n = 8, 8, 4
    sums = np.full((h, w, 3), 3, F); sq = np.full((h, w), 3, F); counts = np.full((h, w), 5, np.uint32); cv = np.full((h, w), 7, np.uint8)
    n_active = C.c_uint32(77)
    good = lambda **kw: api.LightmapParams(*[kw.get(k, v) for k, v in (("model", 0), ("instance", 0), ("w", w), ("h", h), ("first_sample", 0), ("n_samples", n),
                                                                         ("key_base", 0), ("bias", 0.25))])
    direct = lambda base=1000, reserved=0: api.LightmapDirect(base, (C.c_uint32 * 3)(0, reserved, 0))
    crit = api.Adaptive(0.1, 0.0, 2, 0)

    def calls(r):
        error = lambda: r.L.pt_last_error(r.ctx).decode()
        plain = lambda prm, dp, a=sums, b=sq: r.L.pt_bake_lightmap_direct(r.ctx, None if prm is None else C.byref(prm), None if dp is None else C.byref(dp), _p(a), _p(b), _p(cv))
        adaptive = lambda prm, dp, c=crit, a=sums, b=sq, d=counts: r.L.pt_bake_lightmap_adaptive_direct(
            r.ctx, None if prm is None else C.byref(prm), None if dp is None else C.byref(dp), None if c is None else C.byref(c), _p(a), _p(b), _p(d), _p(cv), C.byref(n_active))
        return error, plain, adaptive

    r = api.Renderer(LC.quad_scene(light=True), 48, 32)
    error, plain, adaptive = calls(r)
    # 1. what pt_bake_lightmap_moments / pt_bake_lightmap_adaptive refuse, ahead of a NULL dp
    for prm, code in ((None, ARG), (good(model=-1), ARG), (good(model=2), ARG), (good(instance=1), ARG), (good(w=0), ARG), (good(n_samples=0), ARG),
                      (good(bias=np.nan), ARG), (good(model=1), STATE), (good(w=16385, h=1), LIMIT), (good(key_base=0xFFFFFFFF), ARG)):
        assert plain(prm, None) == code and adaptive(prm, None) == code, (code, error())
    reserved = good()
    reserved.reserved[2] = 1
    assert plain(reserved, None) == ARG and "pt_lightmap_params.reserved" in error()
    assert plain(good(), None, None) == ARG and adaptive(good(), None, crit, sums, None) == ARG and "sumsq" in error()
    assert adaptive(good(), None, None) == ARG and adaptive(good(first_sample=1), None) == ARG and "first_sample" in error()
    assert adaptive(good(), None, api.Adaptive(-1.0, 0.0, 2, 0)) == ARG and "pt_adaptive" in error()
    over = counts.copy(); over[0, 0] = (1 << 24) - n + 1
    assert adaptive(good(), None, crit, sums, sq, over) == LIMIT and "2^24" in error()
    # 2. dp
    for call in (plain, adaptive):
        assert call(good(), None) == ARG and "dp" in error()
        assert call(good(), direct(reserved=1)) == ARG and "pt_lightmap_direct.reserved" in error()
        assert call(good(), direct(base=0xFFFFFFFF - w * h + 2)) == ARG and "light_key_base" in error()
    # 3. no emissive model, whatever enable_nee is; after 2.
    for nee in (True, False):
        dark = api.Renderer(LC.quad_scene(), 48, 32, enable_nee=nee)
        d_error, d_plain, d_adaptive = calls(dark)
        for call in (d_plain, d_adaptive):
            assert call(good(), direct()) == STATE and "emissive" in d_error()
            assert nee or (call(good(), None) == ARG and "dp" in d_error())
    # 4. participating media; 5. the id byte, after 4.
    fog = api.Renderer(_media_scene(), 48, 32)
    f_error, f_plain, f_adaptive = calls(fog)
    for call in (f_plain, f_adaptive):
        assert call(good(), direct()) == STATE and "media" in f_error()
        assert call(good(), direct(reserved=1)) == ARG
    clash = api.Renderer(_many_models(256), 48, 32)
    c_error, c_plain, c_adaptive = calls(clash)
    for call in (c_plain, c_adaptive):
        assert call(good(), direct()) == LIMIT and "low byte" in c_error()
        assert call(good(), None) == ARG
    at_255 = api.Renderer(_many_models(255), 48, 32)
    assert calls(at_255)[1](good(), direct()) == LIMIT and "255" in calls(at_255)[0]()
    assert (sums == 3).all() and (sq == 3).all() and (counts == 5).all() and (cv == 7).all() and n_active.value == 77
    # the lamp moved to model 2, whose low byte no other model has: the same scene passes every check (what follows is the device's: a bake,
    # or no device to run it on).  At model 0 it would share its byte with model 256, as at 256 it shares it with model 0
    lamp_first = _many_models(0)
    lamp_first.models[1].uvs = LC.QUAD_UV[:1]
    assert calls(api.Renderer(lamp_first, 48, 32))[1](good(model=1), direct()) == LIMIT
    fine = api.Renderer(_many_models(2), 48, 32)
    assert calls(fine)[1](good(), direct(), sums.copy(), sq.copy()) in (0, HIP)
    # a key range that ends exactly at 2^32 passes the argument checks
    assert plain(good(), direct(base=(1 << 32) - w * h), sums.copy(), sq.copy()) in (0, HIP)


def test_the_hook_refuses_without_a_light_and_the_wrappers_check_shapes(api):
    dark = api.Renderer(LC.quad_scene(), 48, 32, enable_nee=False)
    with pytest.raises(api.PtError) as e:
        dark.lightmap_light_sample([0], [0], np.zeros((1, 3), F), np.array([[0, 0, 1]], F))
    assert e.value.code == STATE
    r = api.Renderer(LC.quad_scene(light=True), 48, 32)
    with pytest.raises(api.PtError):
        r.lightmap_light_sample([0, 1], [0], np.zeros((2, 3), F), np.zeros((2, 3), F))
    with pytest.raises(api.PtError):
        r.bake_lightmap_direct(0, 0, 8, 8, 4, sums=np.zeros((8, 7, 3), F))
    with pytest.raises(api.PtError):
        r.bake_lightmap_adaptive_direct(0, 0, 8, 8, 4, 0.1, counts=np.zeros((8, 7), np.uint32))
    light, d, t, ce = r.lightmap_light_sample(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3), F), np.zeros((0, 3), F))
    assert light.size == 0 and ce.shape == (0, 3)


# ---- 3. the hook against the restatement
@pytest.mark.parametrize("name", ["quad", "short", "two_lamps", "emtex"])
def test_host_light_sample_is_the_definition(api, oracle_mod, name):
    keys, smp, o, n, want = LD.hook_inputs(oracle_mod, name)
    # the case means something: every lamp triangle is chosen, and rays are cast
    n_lights = {"quad": 2, "short": 2, "two_lamps": 4, "emtex": 2}[name]
    assert (np.bincount(want["light"], minlength=n_lights) > 0).all() and len(np.bincount(want["light"])) == n_lights
    assert want["cast"].any() and (want["ce"][want["cast"]] > 0).any()
    if name == "short":
        # the box's top sees the lamp, its bottom faces away, and the room's ceiling line hides the lamp from part of its sides
        assert (~want["cast"]).any() and (want["blocked"] & want["cast"]).any() and (~want["blocked"] & want["cast"]).any()
    if name == "two_lamps":
        assert len(np.unique(LD.LightTable(LD.oracle_of(oracle_mod, name), LD.case(name)[0]).pdf)) > 1          # unequal areas: unequal pdfs
    if name == "emtex":
        assert len(np.unique(want["ce"][want["cast"]], axis=0)) > 100                                             # the texture varies
    r = LD.renderer(api, name)
    light, d, t, ce = r.lightmap_light_sample(keys, smp, o, n, on_device=False)
    assert np.array_equal(light, want["light"]), name
    assert_bit_equal(d, want["dir"], name + ": dir")
    assert_bit_equal(t, want["t_max"], name + ": t_max")
    assert_bit_equal(ce, want["ce"], name + ": ce")
    assert (ce[~want["cast"]] == 0).all()


def test_some_samples_face_away_from_their_light(oracle_mod):
    assert any((~LD.hook_inputs(oracle_mod, name)[4]["cast"]).any() for name in ("quad", "short", "two_lamps", "emtex"))


# ---- 4. the direct term against the closed form
_CLOSED = {}


def _closed_samples(O):
    """quad_scene(light=True), 8 x 8 texels, 256 samples at bias 0.25: the restated bake's samples, computed once"""
    if "s" not in _CLOSED:
        _CLOSED["s"] = LD.expected_bake(O, "quad", 256, key_base=77, bias=0.25)
    return _CLOSED["s"]


def test_direct_term_is_lamberts_polygon_irradiance(oracle_mod):
    """pi * mean(D) per texel against E = Le / 2 * sum of gamma_e (n . Gamma_e) over the lamp's four edges (binary64), to SIGMAS standard
    errors of the 256 samples' own spread; nothing of the library takes part"""
    s = _closed_samples(oracle_mod)
    n = 256
    assert len(s["k"]) == 64 and not s["clamped"].any() and not s["blocked"].any() and s["cast"].all()
    table = LD.table_of("quad")
    lamp = np.array([[0, 0, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2]], np.float64)
    Dl = s["D"].astype(np.float64).reshape(64, n, 3)
    worst = 0.0
    for j, k in enumerate(s["k"]):
        P = table[2].reshape(-1, 3)[k].astype(np.float64); nr = table[3].reshape(-1, 3)[k].astype(np.float64)
        want = LD.polygon_irradiance(P + np.float64(F(0.25)) * nr, nr, lamp, 5.0)
        for c in range(3):
            got = np.pi * Dl[j, :, c].mean()
            se = np.pi * Dl[j, :, c].std(ddof=1) / np.sqrt(n)
            assert se > 0
            worst = max(worst, abs(got - want) / se)
    print(f"direct term against the closed form: worst deviation {worst:.2f} standard errors over 64 texels x 3 channels")
    assert worst <= SIGMAS, worst


# ---- 5. the whole sample against the plain definition
def test_whole_sample_mean_is_the_plain_gathers(oracle_mod):
    """the map-mean luminance of X against that of the plain gather (Oracle.integrate alone) over the same 64 x 256 rays: the margin is
    SIGMAS standard errors combined from both sides' second moments"""
    s = _closed_samples(oracle_mod)
    lx = LD.lum(s["X"]).astype(np.float64); lp = LD.lum(s["plain"]).astype(np.float64)
    assert s["zeroed"].any() and (~s["zeroed"]).any() and (s["D"] > 0).any()
    se = np.sqrt(lx.var(ddof=1) / len(lx) + lp.var(ddof=1) / len(lp))
    print(f"map-mean luminance: direct {lx.mean():.5f}, plain {lp.mean():.5f}, combined standard error {se:.5f}; per-sample deviation "
          f"direct {lx.std(ddof=1):.4f}, plain {lp.std(ddof=1):.4f}")
    assert abs(lx.mean() - lp.mean()) <= SIGMAS * se, (lx.mean(), lp.mean(), se)
    assert lx.std(ddof=1) < lp.std(ddof=1)          # and that is the point of the estimator
