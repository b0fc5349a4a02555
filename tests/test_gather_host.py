"""CPU: baked rays and the final-gather bake without a GPU: the symbols, every refusal include/pt_api.h promises before any device call, in
its order, and n = 0.  No GPU is touched (the kernels and the bakes: tests/test_gpu_gather.py); a call that passes every check comes back
PT_OK or, with no device to run it on, PT_ERR_HIP."""
import ctypes as C
import os

import numpy as np
import pytest

import lightmap_common as LC
from conftest import ROOT
from test_lightmap_direct_host import _many_models, _media_scene

F = np.float32
ARG, HIP, STATE, LIMIT = -1, -2, -3, -5


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ref(s):
    return None if s is None else C.byref(s)


def _baked(api, hops=2, unlit=(0.25, 0.5, 0.125), reserved=0):
    return api.BakedParams(hops, (C.c_float * 3)(*unlit), (C.c_uint32 * 4)(0, 0, reserved, 0))


# ---- 1. exports
def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in ("pt_baked_rays", "pt_baked_rays_device", "pt_bake_lightmap_gather", "pt_bake_lightmap_adaptive_gather"):
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert C.sizeof(api.BakedRaysParams) == 48 and "} pt_baked_rays_params;" in header
    assert C.sizeof(api.LightmapGather) == 48 and "} pt_lightmap_gather;" in header
    for method in ("baked_rays", "bake_lightmap_gather", "bake_lightmap_adaptive_gather", "bake_lightmaps_gather"):
        assert callable(getattr(api.Renderer, method))
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for name in ("baked_rays(", "bake_lightmap_gather(", "bake_lightmap_adaptive_gather("):
        assert name in wrapper, name
    assert "continuing a path where a chain ends unlit" in header


# ---- 2. baked rays: refusals and n = 0
def test_baked_rays_refusals_fire_in_order_before_any_device_call(api):
    r = api.Renderer(LC.quad_scene(light=True), 48, 32)
    error = lambda: r.L.pt_last_error(r.ctx).decode()
    n = 3
    o = np.zeros((n, 3), F); d = np.tile(np.array([0, 0, -1], F), (n, 1))
    rgbh = np.full((n, 4), 3, F); idb = np.full(n, 7, np.uint8)
    prm = lambda baked=None, window=0, reserved=0: api.BakedRaysParams(baked or _baked(api), window, (C.c_uint32 * 3)(0, reserved, 0))

    def host(p, count=n, oo=o, dd=d, out=rgbh, ids=idb):
        return r.L.pt_baked_rays(r.ctx, count, _p(oo), _p(dd), _ref(p), _p(out), _p(ids))

    def device(p, count=n, oo=o, dd=d):
        return r.L.pt_baked_rays_device(r.ctx, count, _p(oo), _p(dd), _ref(p), None, None)

    for call in (host, device):
        # baked, as pt_render_baked checks it, ahead of everything else
        assert call(None) == ARG and "params" in error()
        assert call(prm(_baked(api, hops=9)), oo=None) == ARG and "max_hops" in error()
        assert call(prm(_baked(api, reserved=1)), oo=None) == ARG and "reserved" in error()
        for bad in ((-1.0, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.inf)):
            assert call(prm(_baked(api, unlit=bad), reserved=1), oo=None) == ARG and "unlit" in error()
        # the call's own reserved words, ahead of the arrays
        assert call(prm(reserved=1), oo=None) == ARG and "pt_baked_rays_params.reserved" in error()
        # NULL arrays with n > 0
        assert call(prm(), oo=None) == ARG and call(prm(), dd=None) == ARG and "o_xyz and d_xyz" in error()
        # n = 0 is PT_OK, with or without arrays, and needs no device
        assert call(prm(), 0) == 0 and call(prm(), 0, None, None) == 0
        assert call(prm(reserved=1), 0) == ARG
    # non-finite components: the host variant reads the rays
    for arr in (o, d):
        for bad in (np.nan, np.inf, -np.inf):
            broken = arr.copy(); broken[1, 2] = bad
            assert host(prm(), **({"oo": broken} if arr is o else {"dd": broken})) == ARG and "ray 1" in error() and "not finite" in error()
    # no camera is needed, and either output may be NULL; what is left is the device's
    assert host(prm()) in (0, HIP) and host(prm(window=64), out=None) in (0, HIP) and host(prm(), ids=None) in (0, HIP)
    if host(prm()) == HIP:
        assert (rgbh == 3).all() and (idb == 7).all()
    # an unbuilt scene, after the parameters and before the arrays
    cfg = api.Config(); cfg.width, cfg.height = 8, 8
    bare = C.c_void_p(r.L.pt_create(C.byref(cfg)))
    assert bare
    try:
        unbuilt = lambda p, oo=o: r.L.pt_baked_rays(bare, n, _p(oo), _p(d), _ref(p), None, None)
        assert unbuilt(prm(reserved=1)) == ARG and unbuilt(prm(), None) == STATE and unbuilt(prm()) == STATE
        assert r.L.pt_baked_rays(bare, 0, None, None, _ref(prm()), None, None) == STATE
    finally:
        r.L.pt_destroy(bare)


# ---- 3. the gather bakes: refusals
def test_gather_refusals_fire_in_order_before_any_device_call_and_nothing_changes(api):
    w, h, n = 8, 8, 4
    sums = np.full((h, w, 3), 3, F); sq = np.full((h, w), 3, F); counts = np.full((h, w), 5, np.uint32); cv = np.full((h, w), 7, np.uint8)
    n_active = C.c_uint32(77)
    good = lambda **kw: api.LightmapParams(*[kw.get(k, v) for k, v in (("model", 0), ("instance", 0), ("w", w), ("h", h), ("first_sample", 0), ("n_samples", n),
                                                                         ("key_base", 0), ("bias", 0.25))])
    gather = lambda direct=1, base=1000, reserved=0, baked=None: api.LightmapGather(baked or _baked(api), direct, base, (C.c_uint32 * 2)(0, reserved))
    crit = api.Adaptive(0.1, 0.0, 2, 0)

    def calls(r):
        error = lambda: r.L.pt_last_error(r.ctx).decode()
        plain = lambda prm, g, a=sums, b=sq: r.L.pt_bake_lightmap_gather(r.ctx, _ref(prm), _ref(g), _p(a), _p(b), _p(cv))
        adaptive = lambda prm, g, c=crit, a=sums, b=sq, d=counts: r.L.pt_bake_lightmap_adaptive_gather(r.ctx, _ref(prm), _ref(g), _ref(c), _p(a), _p(b), _p(d), _p(cv),
                                                                                                    C.byref(n_active))
        return error, plain, adaptive

    r = api.Renderer(LC.quad_scene(light=True), 48, 32)
    error, plain, adaptive = calls(r)
    # 1. what pt_bake_lightmap_moments / pt_bake_lightmap_adaptive refuse, ahead of a NULL g
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
    # 2. g: NULL, then what pt_render_baked refuses in baked, then its own words; each ahead of the next
    for call in (plain, adaptive):
        assert call(good(), None) == ARG and "g must not be NULL" in error()
        assert call(good(), gather(baked=_baked(api, hops=9), reserved=1)) == ARG and "max_hops" in error()
        assert call(good(), gather(baked=_baked(api, reserved=1), reserved=1)) == ARG and "the reserved words" in error()
        assert call(good(), gather(baked=_baked(api, unlit=(0.0, -0.5, 0.0)), reserved=1)) == ARG and "unlit" in error()
        assert call(good(), gather(reserved=1, direct=2)) == ARG and "pt_lightmap_gather.reserved" in error()
        assert call(good(), gather(direct=2)) == ARG and "direct must be 0 or 1" in error()
        assert call(good(), gather(direct=0, base=1)) == ARG and "light_key_base must be 0" in error()
        assert call(good(), gather(base=0xFFFFFFFF - w * h + 2)) == ARG and "light_key_base" in error()
    # 3. direct == 1 refuses what the direct bake refuses; direct == 0 needs no lamp
    for nee in (True, False):
        dark = api.Renderer(LC.quad_scene(), 48, 32, enable_nee=nee)
        d_error, d_plain, d_adaptive = calls(dark)
        for call in (d_plain, d_adaptive):
            if nee:     # (the plain bake's own check comes first)
                assert call(good(), gather(direct=0, base=0)) == STATE and "NEE" in d_error()
            else:
                assert call(good(), gather()) == STATE and "emissive" in d_error()
        if nee:
            continue
        assert d_plain(good(), gather(direct=0, base=0), sums.copy(), sq.copy()) in (0, HIP)
        assert d_adaptive(good(), gather(direct=0, base=0), crit, sums.copy(), sq.copy(), counts.copy()) in (0, HIP)
    # 4. participating media in either mode; 5. the id byte, with direct == 1 only
    fog = api.Renderer(_media_scene(), 48, 32)
    f_error, f_plain, f_adaptive = calls(fog)
    for call in (f_plain, f_adaptive):
        assert call(good(), gather()) == STATE and "media" in f_error()
        assert call(good(), gather(direct=0, base=0)) == STATE and "media" in f_error()
        assert call(good(), gather(reserved=1)) == ARG
    clash = api.Renderer(_many_models(256), 48, 32)
    c_error, c_plain, c_adaptive = calls(clash)
    for call in (c_plain, c_adaptive):
        assert call(good(), gather()) == LIMIT and "low byte" in c_error()
        assert call(good(), None) == ARG
    assert c_plain(good(), gather(direct=0, base=0), sums.copy(), sq.copy()) in (0, HIP)
    assert (sums == 3).all() and (sq == 3).all() and (counts == 5).all() and (cv == 7).all() and n_active.value == 77
    # a call that passes every check, with and without sumsq
    assert plain(good(), gather(), sums.copy(), sq.copy()) in (0, HIP) and plain(good(), gather(), sums.copy(), None) in (0, HIP)
    assert plain(good(), gather(base=(1 << 32) - w * h), sums.copy(), sq.copy()) in (0, HIP)


def test_the_wrappers_check_shapes(api):
    r = api.Renderer(LC.quad_scene(light=True), 48, 32)
    with pytest.raises(api.PtError):
        r.baked_rays(np.zeros((2, 3), F), np.zeros((3, 3), F))
    with pytest.raises(api.PtError):
        r.bake_lightmap_gather(0, 0, 8, 8, 4, sums=np.zeros((8, 7, 3), F))
    with pytest.raises(api.PtError):
        r.bake_lightmap_adaptive_gather(0, 0, 8, 8, 4, 0.1, counts=np.zeros((8, 7), np.uint32))
    with pytest.raises(api.PtError):
        r.bake_lightmaps_gather([(0, 0)], [], 4, 1)
    rgb, hops, idb = r.baked_rays(np.zeros((0, 3), F), np.zeros((0, 3), F), follow=2)
    assert rgb.shape == (0, 3) and hops.shape == (0,) and idb.shape == (0,)
