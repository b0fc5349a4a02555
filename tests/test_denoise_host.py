"""CPU: the edge-aware a-trous denoiser (pt_denoise / pt_post_denoise).  `denoise` below is denoise_common's numpy float32 restatement of the
definition in include/pt_api.h, operation for operation, with exp taken from the oracle's independently written exp_det (math_batch fn 1); the
GPU tests (test_gpu_denoise.py) hold the device to it bit for bit.  Here: hand-computed cases, the model-isolation property, and the library's
argument and state checks, which all run before any device call."""
import ctypes as C

import numpy as np
import pytest

from denoise_common import EPS, MISS, F, _exp, filtered, lum


def denoise(acc, pos, nrm, model, sumsq=None, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0):
    """include/pt_api.h's filter: h x w x 4 accumulation, h x w x 4 position, h x w x 3 normal, h x w model (MISS = 0xffffffff),
    h x w moments or None (spatial variance) -> h x w x 4 (c, 1) / (0, 0, 0, 0)"""
    return filtered(acc, pos, nrm, model, None, sumsq, iterations, sigma_luminance, sigma_normal, sigma_plane)


def random_case(rng, w, h, n_models=6, p_miss=0.15, p_invalid=0.05, spp=4):
    """random accumulation + guides: planes of a few models, misses, unrendered pixels; moments consistent with the sums"""
    model = rng.integers(0, n_models, (h, w)).astype(np.uint32)
    model[rng.random((h, w)) < p_miss] = MISS
    # blocky models so that neighbourhoods hold same-model pixels
    if w > 4 and h > 4:
        model = np.repeat(np.repeat(model[::4, ::4], 4, 0), 4, 1)[:h, :w].copy()
    n = np.full((h, w), F(spp))
    n[rng.random((h, w)) < p_invalid] = 0
    col = rng.random((h, w, 3)).astype(F) * F(2)
    acc = np.concatenate([col * n[..., None], n[..., None]], -1).astype(F)
    nrm = rng.normal(size=(h, w, 3)).astype(F)
    nrm[..., 2] = np.abs(nrm[..., 2]) + F(1.5)             # mostly facing one way: many taps pass the normal term
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    pos = np.concatenate([rng.random((h, w, 3)).astype(F) * F(10), rng.random((h, w, 1)).astype(F) * F(100)], -1).astype(F)
    miss = model == MISS
    nrm[miss] = 0
    pos[miss, 3] = F(1e5)
    q = (lum(acc) * lum(acc) / np.maximum(n, F(1)) * F(1.3)).astype(F)
    return acc, pos, nrm, model, q


# ---------------------------------------------------------------- hand-computed cases
@pytest.fixture(scope="module")
def oracle_built(oracle_mod):
    return oracle_mod


def _img(w, h, colour, n=1.0):
    acc = np.zeros((h, w, 4), F)
    acc[..., :3] = np.asarray(colour, F) * F(n)
    acc[..., 3] = F(n)
    return acc


def test_one_pixel_is_its_own_mean(oracle_built):
    acc = np.array([[[3.0, 1.5, 0.75, 3.0]]], F)
    pos = np.zeros((1, 1, 4), F); nrm = np.array([[[0, 0, 1]]], F); model = np.zeros((1, 1), np.uint32)
    k = F(0.375) * F(0.375)
    c = np.array([1.0, 0.5, 0.25], F)
    want = np.concatenate([(k * c) / k, [F(1)]]).astype(F)
    for sumsq in (None, np.zeros((1, 1), F)):
        out = denoise(acc, pos, nrm, model, sumsq, iterations=3)
        assert np.array_equal(out[0, 0], want)


def test_flat_miss_image_stays_flat_and_invalid_pixels_are_zero(oracle_built):
    """5 x 5 misses of one colour (0.5: every weight times it is exact) at one level: every valid output is (0.5, 1); an unrendered pixel
    with a wild colour is (0, 0, 0, 0) and does not reach its neighbours"""
    W = H = 5
    acc = _img(W, H, (0.5, 0.5, 0.5), 2.0)
    acc[2, 3] = (1e6, -5.0, 7.0, 0.0)
    pos = np.zeros((H, W, 4), F); pos[..., 3] = 1e5
    nrm = np.zeros((H, W, 3), F); model = np.full((H, W), MISS, np.uint32)
    for sumsq in (None, np.full((H, W), F(0.5), F)):
        out = denoise(acc, pos, nrm, model, sumsq, iterations=1)
        assert np.array_equal(out[2, 3], np.zeros(4, F))
        m = np.ones((H, W), bool); m[2, 3] = False
        assert np.array_equal(out[m], np.tile(np.array([0.5, 0.5, 0.5, 1.0], F), (W * H - 1, 1)))


def test_two_misses_with_zero_variance_do_not_mix(oracle_built):
    """zero variance (moments = n * m^2): a tap whose luminance differs from the centre's has weight exp(-huge) = 0"""
    W, H = 5, 4
    acc = _img(W, H, (0.5, 0.5, 0.5), 4.0)
    chk = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(bool)
    acc[chk, :3] = F(0.25) * F(4)
    l = lum(acc) / acc[..., 3]
    q = (l * l * acc[..., 3]).astype(F)                     # Q / n - m^2 == 0 exactly for these values
    pos = np.zeros((H, W, 4), F); nrm = np.zeros((H, W, 3), F); model = np.full((H, W), MISS, np.uint32)
    out = denoise(acc, pos, nrm, model, q, iterations=2)
    assert np.array_equal(out[..., :3], acc[..., :3] / acc[..., 3:4])


def _hand_pair(acc, q):
    """pixel 0 of a 1 x 2 image, one level, moments: inv of its luminance term and |l_0 - l_1| by hand"""
    n = F(1)
    var = []
    for i in range(2):
        a = acc[0, i]
        l = (F(0.2126) * a[0] + F(0.7152) * a[1]) + F(0.0722) * a[2]
        m = l / n
        v = q[0, i] / n - m * m
        var.append((v if v > 0 else F(0)) / n)
    g = (F(0.25) * var[0] + F(0.125) * var[1]) / (F(0.25) + F(0.125))      # 3 x 3 blur: centre 0.5 * 0.5, right 0.5 * 0.25
    inv = F(1) / (F(4) * np.sqrt(g) + EPS)
    c = acc[0, :, :3] / acc[0, :, 3:4]
    l0 = (F(0.2126) * c[0, 0] + F(0.7152) * c[0, 1]) + F(0.0722) * c[0, 2]
    l1 = (F(0.2126) * c[1, 0] + F(0.7152) * c[1, 1]) + F(0.0722) * c[1, 2]
    return inv, np.abs(l0 - l1)


@pytest.mark.parametrize("n_q,stops", [((1.0, 0.0, 0.0), True), ((0.0, 0.0, -1.0), True), ((0.6, 0.0, -0.8), True), ((0.6, 0.0, 0.8), False)])
def test_normals_at_ninety_degrees_and_beyond_stop_the_filter(oracle_built, n_q, stops):
    """two hits of one model at the same point, a large variance (the luminance term lets everything through): the normal term
    max(0, n_p . n_q)^sigma is 0 at 90 degrees and beyond, so each pixel keeps its own colour; at 53 degrees they mix"""
    acc = np.array([[[0.5, 0.5, 0.5, 1.0], [0.25, 0.25, 0.25, 1.0]]], F)
    pos = np.zeros((1, 2, 4), F); pos[..., 3] = 3.0
    nrm = np.array([[[0.0, 0.0, 1.0], n_q]], F)
    model = np.zeros((1, 2), np.uint32)
    q = np.full((1, 2), F(1e4), F)
    out = denoise(acc, pos, nrm, model, q, iterations=1, sigma_normal=1)
    own = np.array_equal(out[0, :, :3], acc[0, :, :3])
    assert own == stops
    if not stops:
        # by hand: centre weight 0.375 * 0.25 (dx = +-1 at step 1 is h[1] = 0.25, dy = 0 is h[2] = 0.375), the other tap's edge weight
        # wn * exp(-(a_x + a_l)) with wn = 0.8, a_x = 0 (same point)
        inv, dl = _hand_pair(acc, q)
        e = F(0.8) * _exp(np.array([-(F(0) + dl * inv)], F))[0]
        w0 = (F(0.375) * F(0.375)) * F(1); w1 = (F(0.25) * F(0.375)) * e
        assert out[0, 0, 0] == (w0 * F(0.5) + w1 * F(0.25)) / (w0 + w1)


def test_plane_distance_term(oracle_built):
    """a neighbour displaced by 1 along the centre's normal (sigma_plane 1): a_x = |n . d| / |d| = 1"""
    acc = np.array([[[0.5, 0.5, 0.5, 1.0], [0.25, 0.25, 0.25, 1.0]]], F)
    pos = np.array([[[0, 0, 0, 1], [0, 0, 1, 1]]], F)
    nrm = np.array([[[0, 0, 1], [0, 0, 1]]], F)
    q = np.full((1, 2), F(1e4), F)
    out = denoise(acc, pos, nrm, np.zeros((1, 2), np.uint32), q, iterations=1)
    inv, dl = _hand_pair(acc, q)
    e = _exp(np.array([-(F(1) + dl * inv)], F))[0]
    w0 = F(0.375) * F(0.375); w1 = (F(0.25) * F(0.375)) * e
    assert out[0, 0, 0] == (w0 * F(0.5) + w1 * F(0.25)) / (w0 + w1)


@pytest.mark.parametrize("moments", [False, True])
def test_models_never_mix(oracle_built, moments):
    """changing every input of one model's pixels leaves every other model's outputs bit-identical"""
    rng = np.random.default_rng(5)
    acc, pos, nrm, model, q = random_case(rng, 29, 23)
    base = denoise(acc, pos, nrm, model, q if moments else None, iterations=3)
    sel = model == 2
    acc2, pos2, nrm2, q2 = acc.copy(), pos.copy(), nrm.copy(), q.copy()
    acc2[sel, :3] *= F(3.5); pos2[sel] += F(1); nrm2[sel] = nrm2[sel][:, ::-1]; q2[sel] *= F(9)
    out = denoise(acc2, pos2, nrm2, model, q2 if moments else None, iterations=3)
    assert np.array_equal(out[~sel].view(np.uint32), base[~sel].view(np.uint32))
    assert not np.array_equal(out[sel], base[sel])


def test_filter_smooths_noise_on_a_flat_model(oracle_built):
    """sanity of the definition: a noisy flat wall of one model gets closer to its mean"""
    rng = np.random.default_rng(1)
    W, H = 24, 16
    col = (F(0.5) + rng.normal(0, 0.1, (H, W, 1)).astype(F)).repeat(3, -1)
    acc = np.concatenate([col, np.ones((H, W, 1), F)], -1).astype(F)
    pos = np.zeros((H, W, 4), F); pos[..., 0] = np.arange(W, dtype=F)[None]; pos[..., 1] = np.arange(H, dtype=F)[:, None]
    nrm = np.zeros((H, W, 3), F); nrm[..., 2] = 1
    out = denoise(acc, pos, nrm, np.zeros((H, W), np.uint32), None)
    assert np.abs(out[..., 0] - 0.5).mean() < 0.5 * np.abs(col[..., 0] - 0.5).mean()


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


def _post(api, r, w=2, h=2, prm=None, drop=None):
    acc = np.ones((h, w, 4), F); pos = np.zeros((h, w, 4), F); nrm = np.zeros((h, w, 3), F); mdl = np.zeros((h, w), np.uint32)
    out = np.zeros((max(h, 1), max(w, 1), 4), F)
    p = api.DenoiseParams(0, 0.0, 0, 0.0) if prm is None else prm
    args = [acc, pos, nrm, mdl]
    ptrs = [None if (drop == i) else a.ctypes.data_as(C.c_void_p) for i, a in enumerate(args)]
    outp = None if drop == 4 else out.ctypes.data_as(C.c_void_p)
    return r.L.pt_post_denoise(r.ctx, w, h, None if drop == "params" else C.byref(p), *ptrs, None, outp)


@pytest.mark.parametrize("prm", [(9, 0.0, 0, 0.0), (0, -1.0, 0, 0.0), (0, float("nan"), 0, 0.0), (0, float("inf"), 0, 0.0), (0, 0.0, 3, 0.0),
                                 (0, 0.0, 512, 0.0), (0, 0.0, 96, 0.0), (0, 0.0, 0, -0.5), (0, 0.0, 0, float("nan"))])
def test_bad_parameters_are_refused_before_the_device(api, renderer, prm):
    p = api.DenoiseParams(*prm)
    assert _post(api, renderer, prm=p) == -1
    assert renderer.L.pt_denoise(renderer.ctx, C.byref(p), None) == -1


@pytest.mark.parametrize("drop", ["params", 0, 1, 2, 3, 4])
def test_null_pointers_are_refused(api, renderer, drop):
    assert _post(api, renderer, drop=drop) == -1


@pytest.mark.parametrize("wh", [(0, 4), (4, 0), (0, 0)])
def test_empty_images_are_refused(api, renderer, wh):
    assert _post(api, renderer, w=wh[0], h=wh[1]) == -1


def test_denoise_needs_guides_and_one_rank(api):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2)
    p = api.DenoiseParams(0, 0.0, 0, 0.0)
    assert r.L.pt_denoise(r.ctx, C.byref(p), None) == -3
    assert "guides" in r.L.pt_last_error(r.ctx).decode()
    assert r.L.pt_read_guides(r.ctx, None, None, None) == -3
    assert r.L.pt_write_denoised_image(r.ctx, b"/nonexistent/x.png") == -3
    r.close()
    r2 = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2, rank=1, world_size=2)
    assert r2.L.pt_denoise(r2.ctx, C.byref(p), None) == -3
    assert "rank" in r2.L.pt_last_error(r2.ctx).decode()
    r2.close()


def test_guides_need_a_scene_and_camera(api):
    cfg = api.Config(8, 8, 2, 0, 0, api.DEFAULT_SEED, 0, 1, 4, 0, -1, 0, 0, 0, 0, 0)
    L = api.lib()
    ctx = C.c_void_p(L.pt_create(C.byref(cfg)))
    assert L.pt_render_guides(ctx, 0) == -3
    L.pt_destroy(ctx)
