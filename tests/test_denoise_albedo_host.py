"""CPU: the demodulated denoiser (pt_denoise_albedo / pt_post_denoise_albedo) and the mean albedo (pt_accumulate_albedo).  The numpy restatement
of include/pt_api.h's definition (denoise_albedo_common.denoise_albedo) is anchored to the existing, trusted restatement of the plain filter
(test_denoise_host.denoise); the GPU tests (test_gpu_denoise_albedo.py) hold the device to it bit for bit.  Here: those anchors, hand cases,
the quality case that motivates the feature, and the library's argument and state checks, which all run before any device call."""
import ctypes as C

import numpy as np
import pytest

from denoise_albedo_common import checker_image, denoise_albedo, random_albedo, rmse
from denoise_common import FLOOR, MISS, F, prepare
from test_denoise_host import denoise, random_case


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------- anchors against test_denoise_host.denoise
@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("what", ["ones", "misses"])
def test_white_albedo_or_all_misses_is_the_plain_filter(oracle_mod, moments, what):
    """(a) k = 1 everywhere: the division, r and the multiplication are exact identities"""
    rng = np.random.default_rng(11)
    acc, pos, nrm, model, q = random_case(rng, 29, 23)
    albedo = random_albedo(rng, 23, 29)
    if what == "ones":
        albedo = np.ones_like(albedo)
    else:
        model = np.full_like(model, MISS); nrm = np.zeros_like(nrm)
    sumsq = q if moments else None
    assert np.array_equal(_u32(denoise_albedo(acc, pos, nrm, model, albedo, sumsq, iterations=3)), _u32(denoise(acc, pos, nrm, model, sumsq, iterations=3)))


def test_spatial_mode_is_the_plain_filter_between_a_division_and_a_product(oracle_mod):
    """(b) without moments nothing but the colour enters the filter"""
    rng = np.random.default_rng(12)
    acc, pos, nrm, model, _ = random_case(rng, 31, 22)
    albedo = random_albedo(rng, 22, 31)
    k = np.where(albedo > FLOOR, albedo, FLOOR).astype(F)
    k[model == MISS] = 1
    acc2 = acc.copy(); acc2[..., :3] = acc[..., :3] / k
    want = denoise(acc2, pos, nrm, model, None, iterations=4)
    want[..., :3] = want[..., :3] * k
    assert np.array_equal(_u32(denoise_albedo(acc, pos, nrm, model, albedo, None, iterations=4)), _u32(want))


@pytest.mark.parametrize("moments", [False, True])
def test_doubling_colour_and_albedo_doubles_the_output(oracle_mod, moments):
    """(c) all hits, albedo above the floor: c' is unchanged, and with moments (Q of the doubled colour is 4 Q) e2 is 4 e2 and r is r / 2, all
    exactly, so var' is unchanged; the last level's product doubles"""
    rng = np.random.default_rng(13)
    acc, pos, nrm, model, q = random_case(rng, 27, 21, p_miss=0.0)
    albedo = (F(0.05) + rng.random((21, 27, 3)).astype(F)).astype(F)
    assert (model != MISS).all() and (albedo > FLOOR).all()
    acc2 = acc.copy(); acc2[..., :3] *= F(2)
    a = denoise_albedo(acc, pos, nrm, model, albedo, q if moments else None, iterations=3)
    b = denoise_albedo(acc2, pos, nrm, model, albedo * F(2), q * F(4) if moments else None, iterations=3)
    want = a.copy(); want[..., :3] *= F(2)
    assert np.array_equal(_u32(b), _u32(want))


@pytest.mark.parametrize("moments", [False, True])
def test_one_models_albedo_does_not_reach_the_others(oracle_mod, moments):
    """(d)"""
    rng = np.random.default_rng(14)
    acc, pos, nrm, model, q = random_case(rng, 29, 23)
    albedo = random_albedo(rng, 23, 29)
    sel = model == 2
    albedo2 = albedo.copy(); albedo2[sel] = albedo2[sel] * F(0.37) + F(0.2)
    sumsq = q if moments else None
    a = denoise_albedo(acc, pos, nrm, model, albedo, sumsq, iterations=3)
    b = denoise_albedo(acc, pos, nrm, model, albedo2, sumsq, iterations=3)
    assert sel.any() and np.array_equal(_u32(a[~sel]), _u32(b[~sel])) and not np.array_equal(a[sel], b[sel])


# ---------------------------------------------------------------- hand cases
def _flat(w, h, rgb, n=2.0):
    acc = np.zeros((h, w, 4), F); acc[..., :3] = np.asarray(rgb, F) * F(n); acc[..., 3] = F(n)
    pos = np.zeros((h, w, 4), F); pos[..., 0] = np.arange(w, dtype=F)[None]; pos[..., 3] = 2
    nrm = np.zeros((h, w, 3), F); nrm[..., 2] = 1
    return acc, pos, nrm, np.zeros((h, w), np.uint32)


@pytest.mark.parametrize("moments", [False, True])
def test_zero_albedo_channel_takes_the_floor(oracle_mod, moments):
    """albedo green 0 on a hit: k.g = 2^-10, so the output there is the filtered irradiance / 1024 and never above the largest input irradiance
    / 1024 (the filter's weights are a convex combination); the other channels are divided and multiplied by their own albedo"""
    W, H = 6, 5
    acc, pos, nrm, model = _flat(W, H, (0.5, 0.25, 0.5))
    acc[..., 1] = (F(0.25) + F(0.125) * np.random.default_rng(3).random((H, W)).astype(F)) * acc[..., 3]
    albedo = np.zeros((H, W, 3), F); albedo[..., 0] = 0.5; albedo[..., 2] = 0.25
    q = np.full((H, W), F(1.0), F) if moments else None
    cd, _, k, _ = prepare(acc, model, albedo, q)
    assert (k[..., 1] == FLOOR).all() and np.array_equal(cd[..., 1], (acc[..., 1] * F(1024)) / acc[..., 3])
    out = denoise_albedo(acc, pos, nrm, model, albedo, q, iterations=2)
    assert (out[..., 1] <= cd[..., 1].max() / F(1024)).all() and (out[..., 1] >= cd[..., 1].min() / F(1024)).all()
    assert np.array_equal(out[..., 0], np.full((H, W), F(0.5))) and np.array_equal(out[..., 2], np.full((H, W), F(0.5)))
    # a miss with the same albedo is not divided at all
    miss = np.full_like(model, MISS)
    assert (prepare(acc, miss, albedo, q)[2] == 1).all()


def test_black_pixel_keeps_its_variance(oracle_mod):
    """l(c) == 0: r = 1, var' = e2 (no 0 / 0), and the output stays black and finite"""
    acc, pos, nrm, model = _flat(3, 1, (0.5, 0.5, 0.5), 4.0)
    acc[0, 1, :3] = 0
    q = np.full((1, 3), F(6.0), F)
    albedo = np.full((1, 3, 3), F(0.25), F)
    cd, var, _, _ = prepare(acc, model, albedo, q)
    assert var[0, 1] == (F(6.0) / F(4.0)) / F(4.0) and np.array_equal(cd[0, 1], np.zeros(3, F))
    # the lit neighbours: r = l(c') / l(c) with c = 0.5 and c' = 2
    m = ((F(0.2126) * F(2) + F(0.7152) * F(2)) + F(0.0722) * F(2)) / F(4.0)
    e2 = (F(6.0) / F(4.0) - m * m) / F(4.0)
    lc = (F(0.2126) * F(0.5) + F(0.7152) * F(0.5)) + F(0.0722) * F(0.5)
    lcd = (F(0.2126) * F(2) + F(0.7152) * F(2)) + F(0.0722) * F(2)
    assert var[0, 0] == (e2 * (lcd / lc)) * (lcd / lc)
    out = denoise_albedo(acc, pos, nrm, model, albedo, q, iterations=2)
    assert np.isfinite(out).all() and (out[..., 3] == 1).all()


@pytest.mark.parametrize("moments", [False, True])
def test_invalid_pixel_is_zero_and_no_neighbour(oracle_mod, moments):
    W, H = 5, 5
    acc, pos, nrm, model = _flat(W, H, (0.5, 0.5, 0.5))
    acc[2, 3] = (1e6, -5.0, 7.0, 0.0)
    albedo = np.full((H, W, 3), F(0.5), F); albedo[2, 3] = (0.0, 2.0, 1e-9)
    out = denoise_albedo(acc, pos, nrm, model, albedo, np.full((H, W), F(0.5), F) if moments else None, iterations=2)
    assert np.array_equal(out[2, 3], np.zeros(4, F))
    m = np.ones((H, W), bool); m[2, 3] = False
    assert np.array_equal(out[m], np.tile(np.array([0.5, 0.5, 0.5, 1.0], F), (W * H - 1, 1)))


# ---------------------------------------------------------------- the quality case
def test_demodulation_keeps_a_checker_the_plain_filter_destroys(oracle_mod):
    """48 x 32, one model, 4-pixel checker albedo times a smooth irradiance ramp, 4 noisy samples, spatial variance.  Measured: input 0.155,
    plain filter 0.294 (worse than not denoising), demodulated 0.022"""
    acc, pos, nrm, model, albedo, truth = checker_image()
    noisy = rmse(acc[..., :3] / acc[..., 3:4], truth)
    plain = rmse(denoise(acc, pos, nrm, model, None), truth)
    demod = rmse(denoise_albedo(acc, pos, nrm, model, albedo, None), truth)
    print(f"checker rmse: input {noisy:.4f} plain {plain:.4f} demodulated {demod:.4f}")
    assert demod < 0.5 * noisy and demod < 0.5 * plain


# ---------------------------------------------------------------- argument and state checks (no device needed)
@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


@pytest.fixture()
def renderer(api):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2)
    yield r
    r.close()


NEW = ["pt_accumulate_albedo", "pt_reset_albedo", "pt_read_albedo", "pt_denoise_albedo", "pt_post_denoise_albedo"]


def test_the_entry_points_are_exported_and_declared(api):
    import os
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    assert (api.ALBEDO_GUIDE, api.ALBEDO_MEAN) == (1, 2) and "PT_ALBEDO_GUIDE = 1, PT_ALBEDO_MEAN = 2" in header


def _post(api, r, w=2, h=2, prm=None, drop=None, albedo=None):
    acc = np.ones((h, w, 4), F); pos = np.zeros((h, w, 4), F); nrm = np.zeros((h, w, 3), F); mdl = np.zeros((h, w), np.uint32)
    al = np.ones((max(h, 1), max(w, 1), 3), F) if albedo is None else np.ascontiguousarray(albedo, F)
    out = np.zeros((max(h, 1), max(w, 1), 4), F)
    p = api.DenoiseParams(0, 0.0, 0, 0.0) if prm is None else prm
    ptrs = [None if (drop == i) else a.ctypes.data_as(C.c_void_p) for i, a in enumerate([acc, pos, nrm, mdl, al])]
    outp = None if drop == 5 else out.ctypes.data_as(C.c_void_p)
    return r.L.pt_post_denoise_albedo(r.ctx, w, h, None if drop == "params" else C.byref(p), *ptrs, None, outp)


@pytest.mark.parametrize("prm", [(9, 0.0, 0, 0.0), (0, -1.0, 0, 0.0), (0, float("nan"), 0, 0.0), (0, float("inf"), 0, 0.0), (0, 0.0, 3, 0.0),
                                 (0, 0.0, 512, 0.0), (0, 0.0, 96, 0.0), (0, 0.0, 0, -0.5), (0, 0.0, 0, float("nan"))])
def test_bad_parameters_are_refused_before_the_device(api, renderer, prm):
    p = api.DenoiseParams(*prm)
    assert _post(api, renderer, prm=p) == -1
    for source in (api.ALBEDO_GUIDE, api.ALBEDO_MEAN):
        assert renderer.L.pt_denoise_albedo(renderer.ctx, C.byref(p), source, None) == -1


@pytest.mark.parametrize("drop", ["params", 0, 1, 2, 3, 4, 5])
def test_null_pointers_are_refused(api, renderer, drop):
    assert _post(api, renderer, drop=drop) == -1


@pytest.mark.parametrize("wh", [(0, 4), (4, 0), (0, 0)])
def test_empty_images_are_refused(api, renderer, wh):
    assert _post(api, renderer, w=wh[0], h=wh[1]) == -1


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf")])
def test_bad_albedo_is_refused(api, renderer, bad):
    al = np.ones((2, 2, 3), F); al[1, 0, 2] = bad
    assert _post(api, renderer, albedo=al) == -1
    assert "pixel 2" in renderer.L.pt_last_error(renderer.ctx).decode()
    with pytest.raises(api.PtError) as e:
        renderer.post_denoise_albedo(np.ones((2, 2, 4), F), np.zeros((2, 2, 4), F), np.zeros((2, 2, 3), F), np.zeros((2, 2), np.uint32), al)
    assert e.value.code == -1
    with pytest.raises(api.PtError):      # the wrapper's own shape check
        renderer.post_denoise_albedo(np.ones((2, 2, 4), F), np.zeros((2, 2, 4), F), np.zeros((2, 2, 3), F), np.zeros((2, 2), np.uint32), np.ones((2, 3, 3), F))


@pytest.mark.parametrize("source", [0, 3, 0xFFFFFFFF])
def test_bad_albedo_source_is_refused(api, renderer, source):
    p = api.DenoiseParams(0, 0.0, 0, 0.0)
    assert renderer.L.pt_denoise_albedo(renderer.ctx, C.byref(p), source, None) == -1
    assert "albedo_source" in renderer.L.pt_last_error(renderer.ctx).decode()


def test_denoise_albedo_needs_guides_and_one_rank(api):
    from path_tracer_amd import scenes
    p = api.DenoiseParams(0, 0.0, 0, 0.0)
    r = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2)
    for source in (api.ALBEDO_GUIDE, api.ALBEDO_MEAN):
        assert r.L.pt_denoise_albedo(r.ctx, C.byref(p), source, None) == -3
        assert "guides" in r.L.pt_last_error(r.ctx).decode()
    with pytest.raises(api.PtError) as e:
        r.denoise_albedo()
    assert e.value.code == -3
    r.close()
    r2 = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2, rank=1, world_size=2)
    assert r2.L.pt_denoise_albedo(r2.ctx, C.byref(p), api.ALBEDO_MEAN, None) == -3
    assert "rank" in r2.L.pt_last_error(r2.ctx).decode()
    r2.close()


def test_mean_albedo_argument_and_state_checks(api, renderer):
    L, ctx = renderer.L, renderer.ctx
    assert L.pt_read_albedo(ctx, None) == -3 and "albedo" in L.pt_last_error(ctx).decode()
    assert L.pt_accumulate_albedo(ctx, 0, 0) == -1
    assert L.pt_accumulate_albedo(ctx, 2, 0xFFFFFFFF) == -1          # one sample beyond 2^32
    assert L.pt_accumulate_albedo(ctx, 0xFFFFFFFF, 2) == -1
    assert L.pt_reset_albedo(ctx) == 0
    assert L.pt_read_albedo(ctx, None) == -3
    with pytest.raises(api.PtError) as e:
        renderer.read_albedo()
    assert e.value.code == -3
    assert L.pt_reset_albedo(None) == -1 and L.pt_read_albedo(None, None) == -1 and L.pt_accumulate_albedo(None, 0, 1) == -1


def test_mean_albedo_needs_a_scene_and_camera(api):
    cfg = api.Config(8, 8, 2, 0, 0, api.DEFAULT_SEED, 0, 1, 4, 0, -1, 0, 0, 0, 0, 0)
    L = api.lib()
    ctx = C.c_void_p(L.pt_create(C.byref(cfg)))
    assert L.pt_accumulate_albedo(ctx, 0, 1) == -3
    assert L.pt_accumulate_albedo(ctx, 0, 0) in (-1, -3)
    L.pt_destroy(ctx)
