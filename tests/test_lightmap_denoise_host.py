"""CPU: the texel-space denoiser (pt_lightmap_denoise with on_device = 0, pt_bake_lightmap_moments' refusals) without a GPU: the symbols, the host
walk bit for bit against the numpy restatement of tests/lightmap_denoise_common.py and, with the reach switched off, against denoise_common's
frame filter on the equivalent images; chart independence, coverage, and every refusal include/pt_api.h promises before any device call (asked
with on_device = 1 too: this machine has no GPU to answer).  No GPU is touched (the kernels and the bake: tests/test_gpu_lightmap_denoise.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_common as DC
import lightmap_common as LC
import lightmap_denoise_common as LD
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, STATE, LIMIT = -1, -3, -5
OFF = 1e30          # reach * reach overflows: the term is off


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_RENDERERS = {}


def renderer(api, kind):
    if kind not in _RENDERERS:
        _RENDERERS[kind] = api.Renderer(LD.scene(kind)[0], 48, 32)
    return _RENDERERS[kind]


def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in ("pt_bake_lightmap_moments", "pt_lightmap_denoise"):
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert "typedef struct pt_lightmap_denoise_params" in header
    assert C.sizeof(api.LightmapDenoiseParams) == 56
    for method in ("bake_lightmap_moments", "denoise_lightmap"):
        assert callable(getattr(api.Renderer, method))
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    assert "bake_lightmap_moments(" in wrapper and "denoise_lightmap(" in wrapper


# ---- the restatement
@pytest.mark.parametrize("kind, w, h, it, moments", LD.case_ids())
def test_host_filter_is_the_definition(api, kind, w, h, it, moments):
    table, sums, sumsq, (want, want_area) = LD.expected(kind, w, h, it, moments)
    covered = table[0] != LC.MISS
    assert covered.any() and (kind != "box" or not covered.all())
    got, area = renderer(api, kind).denoise_lightmap(LD.scene(kind)[1], 0, sums, LD.N_SAMPLES, sumsq=sumsq, iterations=it, on_device=False, want_area=True)
    assert_bit_equal(area, want_area, "texel area")
    assert (area[covered] > 0).all() and not area[~covered].any()
    assert_bit_equal(got, want, f"{kind} {w}x{h}, {it} levels, moments {moments}")
    if w * h > 1:
        assert np.abs(got[covered] - (sums / F(LD.N_SAMPLES))[covered]).max() > 0          # it filtered


def test_the_reach_rejects_taps_the_frame_filter_takes():
    """the grid above cannot pass on a filter without the term: on TWO-CHART the restatement under the default reach differs from the one with
    the term off"""
    _, _, _, (near, _) = LD.expected("two", 16, 16, 3, True)
    _, _, _, (far, _) = LD.expected("two", 16, 16, 3, True, reach=OFF)
    assert (near != far).any()


# ---- equivalence
@pytest.mark.parametrize("kind, w, h", [("box", 37, 19), ("two", 16, 16), ("quad", 1, 1)])
@pytest.mark.parametrize("moments", [True, False])
def test_without_reach_it_is_the_frame_filter(api, kind, w, h, moments):
    table = LD.table_of(kind, w, h)
    sums, sumsq = LD.synthetic(w, h, LD.N_SAMPLES, seed=5)
    sq = sumsq if moments else None
    acc, pos, nrm, model = LD.frame_images(table, sums, LD.N_SAMPLES)
    want = DC.filtered(acc, pos, nrm, model, None, sq, 4, 0.0, 0, 0.0)
    got = renderer(api, kind).denoise_lightmap(LD.scene(kind)[1], 0, sums, LD.N_SAMPLES, sumsq=sq, iterations=4, reach=OFF, on_device=False)
    assert_bit_equal(got, want[..., :3], f"{kind} {w}x{h} moments {moments}: reach off")


# ---- chart independence
def test_charts_do_not_exchange_light(api):
    r = renderer(api, "two")
    table = LD.table_of("two", 16, 16)
    in_a, in_b = LD.chart_masks(table[0])
    assert in_a.sum() == 7 * 16 and in_b.sum() == 8 * 16 and not (table[0][:, 7] != LC.MISS).any()
    sums, sumsq = LD.synthetic(16, 16, LD.N_SAMPLES, seed=9)
    other = sums.copy()
    other[in_b] = LD.synthetic(16, 16, LD.N_SAMPLES, seed=10)[0][in_b] * F(3)
    for moments in (sumsq, None):
        base = r.denoise_lightmap(0, 0, sums, LD.N_SAMPLES, sumsq=moments, on_device=False)
        moved = r.denoise_lightmap(0, 0, other, LD.N_SAMPLES, sumsq=moments, on_device=False)
        assert_bit_equal(moved[in_a], base[in_a], "chart A under the default reach")
        assert (moved[in_b] != base[in_b]).any()
        assert np.abs(base[in_a] - (sums / F(LD.N_SAMPLES))[in_a]).max() > 0                # ... and chart A was filtered
        base = r.denoise_lightmap(0, 0, sums, LD.N_SAMPLES, sumsq=moments, reach=OFF, on_device=False)
        moved = r.denoise_lightmap(0, 0, other, LD.N_SAMPLES, sumsq=moments, reach=OFF, on_device=False)
        assert (moved[in_a] != base[in_a]).any(), "with the reach off the coplanar charts leak"


# ---- coverage
def test_uncovered_texels_are_zero_and_are_never_read(api):
    r = renderer(api, "box")
    model = LD.scene("box")[1]
    table = LD.table_of("box", 37, 19)
    covered = table[0] != LC.MISS
    sums, sumsq = LD.synthetic(37, 19, LD.N_SAMPLES, seed=3)
    other, other_sq = sums.copy(), sumsq.copy()
    other[~covered] = F(1000); other_sq[~covered] = F(7)
    for moments in (True, False):
        base = r.denoise_lightmap(model, 0, sums, LD.N_SAMPLES, sumsq=sumsq if moments else None, on_device=False)
        assert not base[~covered].any() and (base[covered] > 0).all()
        got = r.denoise_lightmap(model, 0, other, LD.N_SAMPLES, sumsq=other_sq if moments else None, on_device=False)
        assert_bit_equal(got, base, "uncovered inputs changed")


# ---- errors
def _call(r, on_device, prm, sums, sumsq, out, area=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return r.L.pt_lightmap_denoise(r.ctx, on_device, None if prm is None else C.byref(prm), p(sums), p(sumsq), p(out), p(area))


def test_arguments_are_refused_before_any_device_call_and_nothing_changes(api):
    r = renderer(api, "box")
    model = LD.scene("box")[1]
    w, h = 12, 8
    sums, sumsq = LD.synthetic(w, h, 16, seed=1)
    out = np.full((h, w, 3), 7, F); area = np.full((h, w), 7, F)

    def prm(**kw):
        v = dict(model=model, instance=0, w=w, h=h, n_samples=16, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, reach=0.0)
        v.update(kw)
        return api.LightmapDenoiseParams(v["model"], v["instance"], v["w"], v["h"], v["n_samples"],
                                         api.DenoiseParams(v["iterations"], v["sigma_luminance"], v["sigma_normal"], v["sigma_plane"]), v["reach"])

    def bad(a, value, at=5):
        b = a.copy()
        b.reshape(-1)[at] = value
        return b

    big = np.zeros(1, F)          # never read: each of these is refused for its sizes alone
    refusals = [
        (prm(model=-1), ARG), (prm(model=6), ARG), (prm(instance=1), ARG), (prm(w=0), ARG), (prm(h=0), ARG), (prm(model=0), STATE),
        (prm(w=16385, h=1), LIMIT), (prm(w=1, h=16385), LIMIT), (prm(w=16384, h=8192), LIMIT),
        (prm(iterations=9), ARG), (prm(sigma_luminance=-1.0), ARG), (prm(sigma_luminance=np.nan), ARG), (prm(sigma_luminance=np.inf), ARG),
        (prm(sigma_plane=-1.0), ARG), (prm(sigma_plane=np.nan), ARG), (prm(sigma_plane=np.inf), ARG), (prm(sigma_normal=3), ARG), (prm(sigma_normal=512), ARG),
        (prm(n_samples=0), ARG), (prm(n_samples=(1 << 24) + 1), ARG), (prm(reach=-1.0), ARG), (prm(reach=np.nan), ARG), (prm(reach=np.inf), ARG),
    ]
    for on_device in (0, 1):
        for p, code in refusals:
            target = big if (p.w, p.h) != (w, h) else sums
            assert _call(r, on_device, p, target, None, out, area) == code, (on_device, p.model, p.instance, p.w, p.h, p.n_samples, p.reach, code)
        for word in range(4):
            p = prm()
            p.reserved[word] = 1
            assert _call(r, on_device, p, sums, sumsq, out, area) == ARG
        assert _call(r, on_device, None, sums, sumsq, out) == ARG
        assert _call(r, on_device, prm(), None, sumsq, out) == ARG
        assert _call(r, on_device, prm(), sums, sumsq, None) == ARG
        for value in (-1.0, np.nan, np.inf, -np.inf):
            assert _call(r, on_device, prm(), bad(sums, value), sumsq, out, area) == ARG, value
            assert _call(r, on_device, prm(), sums, bad(sumsq, value), out, area) == ARG, value
            assert _call(r, on_device, prm(), bad(sums, value, at=w * h * 3 - 1), None, out, area) == ARG, value
    assert "sumsq" not in r.L.pt_last_error(r.ctx).decode() and "rgb_sum" in r.L.pt_last_error(r.ctx).decode()
    assert (out == 7).all() and (area == 7).all()
    # the ends of the ranges themselves are fine, and the host path then runs
    assert _call(r, 0, prm(n_samples=1 << 24, iterations=8, sigma_normal=256, reach=1e30), sums, sumsq, out, None) == 0
    assert not (out == 7).all()
    with pytest.raises(api.PtError) as e:
        r.denoise_lightmap(model, 3, sums, 16, on_device=False)
    assert e.value.code == ARG


def test_moments_bake_arguments_are_refused(api):
    r = renderer(api, "box")
    model = LD.scene("box")[1]
    w, h = 12, 8
    sums = np.full((h, w, 3), 3, F); sq = np.full((h, w), 3, F); cov = np.full((h, w), 7, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    bake = lambda prm, a, b: r.L.pt_bake_lightmap_moments(r.ctx, None if prm is None else C.byref(prm), p(a), p(b), p(cov))
    good = api.LightmapParams(model, 0, w, h, 0, 4, 0, 0.25)
    assert bake(good, sums, None) == ARG and "sumsq" in r.L.pt_last_error(r.ctx).decode()
    assert bake(good, None, sq) == ARG and bake(None, sums, sq) == ARG
    for prm, code in ((api.LightmapParams(-1, 0, w, h, 0, 4, 0, 0.25), ARG), (api.LightmapParams(model, 0, w, h, 0, 0, 0, 0.25), ARG),
                      (api.LightmapParams(model, 0, w, h, 0, 4, 0, np.nan), ARG), (api.LightmapParams(0, 0, w, h, 0, 4, 0, 0.25), STATE),
                      (api.LightmapParams(model, 0, 16385, 1, 0, 4, 0, 0.25), LIMIT)):
        assert bake(prm, sums, sq) == code
    reserved = api.LightmapParams(model, 0, w, h, 0, 4, 0, 0.25)
    reserved.reserved[2] = 1
    assert bake(reserved, sums, sq) == ARG
    assert (sums == 3).all() and (sq == 3).all() and (cov == 7).all()
