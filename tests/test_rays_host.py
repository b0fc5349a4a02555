"""CPU: caller-supplied rays and irradiance probes (pt_integrate_rays, pt_integrate_rays_device, pt_bake_probes, pt_probe_ray): the symbols,
every refusal that include/pt_api.h promises before any device call, and pt_probe_ray against a numpy restatement.  No GPU is touched.

`probe_rays` restates the probe definition of include/pt_api.h in numpy binary32, one rounding per operation, with the oracle's own stream
draws, Sobol points and sin/cos; tests/test_gpu_rays.py feeds its directions to the oracle's integrator for the expected coefficients."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal

F = np.float32
SEED = 0x5EED5EED
ARG, STATE = -1, -3
NEW_SYMBOLS = ["pt_integrate_rays", "pt_integrate_rays_device", "pt_bake_probes", "pt_probe_ray"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


@pytest.fixture(scope="module")
def renderer(api):
    from path_tracer_amd import scenes
    return api.Renderer(scenes.cornell_box(48, 32), 48, 32)


def probe_sh9(d):
    """y0..y8 of directions d [n, 3] (binary32, the header's order of operations)"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c1, c2 = F(0.48860252), F(1.0925484)
    out = np.stack([np.full(len(d), F(0.2820948), F), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z),
                    F(0.31539157) * (F(3.0) * (z * z) - F(1.0)), c2 * (x * z), F(0.54627424) * (x * x - y * y)], 1)
    assert out.dtype == F
    return out


def probe_rays(O, keys, samples, n_sobol=512, seed=SEED):
    """directions [n, 3] and basis values [n, 9] of the probe samples (key[i], sample[i]): include/pt_api.h, pt_bake_probes, line for line"""
    L = O.lib()
    n = len(keys)
    u = np.zeros((n, 2), F)
    for i, (k, s) in enumerate(zip(keys, samples)):
        seed0 = int(L.pto_wyrand(int(L.pto_stream_state0(seed, int(k), int(s))), 0)) & 0xFFFFFFFF
        u[i] = O.ss_sobol(n_sobol, int(s), seed0)
    z = F(1.0) - F(2.0) * u[:, 0]
    r2 = F(1.0) - z * z
    r = np.sqrt(np.where(r2 > 0, r2, F(0.0)).astype(F))
    phi = F(6.2831855) * u[:, 1]
    sn, cs = O.math_batch(0, phi)
    d = np.stack([r * cs, r * sn, z], 1)
    assert d.dtype == F
    return d, probe_sh9(d)


def test_symbols_are_exported_and_bound(api):
    L = api.lib()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    for method in ("integrate_rays", "bake_probes", "probe_ray"):
        assert callable(getattr(api.Renderer, method))
    assert C.sizeof(api.RaysParams) == 16 and C.sizeof(api.ProbeParams) == 16


def _rays(n):
    o = np.tile(np.array([278.0, 273.0, -300.0], F), (n, 1))
    d = np.tile(np.array([0.0, 0.0, 1.0], F), (n, 1))
    return o, d, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32)


def _call_rays(api, r, fn, n, o, d, key, sample, prm, outs=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rad = np.zeros((max(n, 1), 4), F); pos = np.zeros((max(n, 1), 4), F); idb = np.zeros(max(n, 1), np.uint8)
    code = getattr(r.L, fn)(r.ctx, n, p(o), p(d), p(key), p(sample), None if prm is None else C.byref(prm), p(rad) if outs else None,
                            p(pos) if outs else None, p(idb) if outs else None)
    return code, r.L.pt_last_error(r.ctx).decode()


@pytest.mark.parametrize("fn", ["pt_integrate_rays", "pt_integrate_rays_device"])
def test_ray_arguments_are_refused_before_any_device_call(api, renderer, fn):
    r = renderer
    o, d, key, sample = _rays(8)
    ok = api.RaysParams(1, 0)
    for missing in range(5):
        args = [o, d, key, sample, ok]
        args[missing] = None
        code, _ = _call_rays(api, r, fn, 8, *args)
        assert code == ARG, (fn, missing, code)
    for word in range(2):
        bad = api.RaysParams(1, 0)
        bad.reserved[word] = 1
        assert _call_rays(api, r, fn, 8, o, d, key, sample, bad)[0] == ARG
    # nothing to do is not an error, with or without pointers
    assert _call_rays(api, r, fn, 0, None, None, None, None, None, outs=False)[0] == 0
    assert _call_rays(api, r, fn, 0, o, d, key, sample, ok)[0] == 0


def test_non_finite_rays_are_named(api, renderer):
    o, d, key, sample = _rays(8)
    for arr, what, row, col, value in ((o, "o", 5, 1, np.nan), (d, "d", 3, 2, np.inf), (d, "d", 0, 0, -np.inf), (o, "o", 7, 0, np.inf)):
        a = arr.copy()
        a[row, col] = value
        if row < 7:
            a[7, 2] = np.nan        # a later one: the message names the FIRST
        args = (a, d) if arr is o else (o, a)
        code, msg = _call_rays(api, renderer, "pt_integrate_rays", 8, *args, key, sample, api.RaysParams(1, 0))
        assert code == ARG and f"ray {row} " in msg and f" {what} " in msg, (code, msg)
    with pytest.raises(api.PtError) as e:
        bad = o.copy(); bad[2, 0] = np.nan
        renderer.integrate_rays(bad, d, key, sample)
    assert e.value.code == ARG and "ray 2 " in str(e.value)


def test_rays_and_probes_need_a_built_scene_but_no_camera(api):
    L = api.lib()
    cfg = api.Config(48, 32, 8, 512, 1, SEED, 0, 1, 4, 0, -1, 0, 0, 0, 0, 0)
    ctx = C.c_void_p(L.pt_create(C.byref(cfg)))
    try:
        o, d, key, sample = _rays(4)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        prm = api.RaysParams(1, 0)
        for fn in ("pt_integrate_rays", "pt_integrate_rays_device"):
            assert getattr(L, fn)(ctx, 4, p(o), p(d), p(key), p(sample), C.byref(prm), None, None, None) == STATE
            assert getattr(L, fn)(ctx, 0, None, None, None, None, None, None, None, None) == STATE
        sh = np.zeros(27, F)
        pp = api.ProbeParams(0, 4, 0, 0)
        assert L.pt_bake_probes(ctx, 1, p(o), C.byref(pp), p(sh)) == STATE
    finally:
        L.pt_destroy(ctx)
    # a built scene without a camera passes the state check (and is then refused for its arguments, still without a device)
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import SceneDesc
    sc = scenes.cornell_box(48, 32)
    r = api.Renderer(SceneDesc.new(sc.models, None, sc.name), 48, 32)
    assert _call_rays(api, r, "pt_integrate_rays", 4, None, d, key, sample, prm)[0] == ARG
    assert _call_rays(api, r, "pt_integrate_rays", 0, None, None, None, None, None, outs=False)[0] == 0


def test_probe_arguments_are_refused_before_any_device_call(api, renderer):
    r, L = renderer, renderer.L
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pos = np.array([[278.0, 273.0, 280.0], [100.0, 100.0, 100.0]], F)
    sh = np.zeros((2, 27), F)

    def call(n, position, prm, out):
        return L.pt_bake_probes(r.ctx, n, p(position), None if prm is None else C.byref(prm), p(out))

    ok = api.ProbeParams(0, 4, 0, 0)
    assert call(2, None, ok, sh) == ARG
    assert call(2, pos, None, sh) == ARG
    assert call(2, pos, ok, None) == ARG
    assert call(2, pos, api.ProbeParams(0, 0, 0, 0), sh) == ARG                      # n_samples == 0
    assert call(2, pos, api.ProbeParams(0, 4, 0, 1), sh) == ARG                      # reserved
    assert call(2, pos, api.ProbeParams(0, 4, 0xFFFFFFFF, 0), sh) == ARG             # key_base + n_probes wraps
    assert call(2, pos, api.ProbeParams(0xFFFFFFFE, 3, 0, 0), sh) == ARG             # first_sample + n_samples wraps
    for value in (np.nan, np.inf):
        bad = pos.copy(); bad[1, 2] = value
        assert call(2, bad, ok, sh) == ARG
        assert "probe 1 " in L.pt_last_error(r.ctx).decode()
    assert call(0, None, None, None) == 0
    assert not sh.any()


def test_probe_ray_is_the_definition(api, oracle_mod, renderer):
    """4 096 (key, sample) pairs, keys up to 2^32 - 1 and samples beyond n_sobol = 512"""
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
    keys[:4] = (0, 1, 0x80000000, 0xFFFFFFFF)
    samples = rng.integers(0, 4000, 4096, dtype=np.uint64)
    samples[:4] = (0, 511, 512, 0xFFFFFFFF)
    assert (keys >= 1 << 31).sum() > 1000 and (samples >= 512).sum() > 1000
    want_d, want_y = probe_rays(oracle_mod, keys, samples)
    got_d = np.zeros((4096, 3), F); got_y = np.zeros((4096, 9), F)
    for i in range(4096):
        got_d[i], got_y[i] = renderer.probe_ray(int(keys[i]), int(samples[i]))
    assert_bit_equal(got_d, want_d, "probe directions")
    assert_bit_equal(got_y, want_y, "probe basis values")
    length = np.sqrt((got_d.astype(np.float64) ** 2).sum(1))
    assert np.abs(length - 1.0).max() < 1e-6, np.abs(length - 1.0).max()


def test_probe_directions_cover_the_sphere(api, renderer):
    """the first 4 096 samples of one key: a shuffled-scrambled Sobol sequence through an area-preserving map, so the mean direction is near 0"""
    d = np.array([renderer.probe_ray(77, s)[0] for s in range(4096)], np.float64)
    mean = d.mean(0)
    assert np.abs(mean).max() < 0.05, mean
    assert (d[:, 2] > 0).sum() in range(1900, 2200) and (d[:, 0] > 0).sum() in range(1900, 2200)
