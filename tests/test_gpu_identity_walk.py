"""GPU (-m gpu): the one-ray walk of identity-only scenes (IDENT kernels, ident_ray in pt_kernels.hip) against the general two-level
walk (PT_FLAG_GENERAL_WALK) and the CPU oracle, on the rays where the two could part: signed zeros, infinities and NaNs."""
import dataclasses

import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _ident_tlas(r):
    r.trace_any(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32), np.ones(1, np.float32))   # the scene is resident
    return r.stats().ident_tlas


def _edge_rays():
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, 1e-40, -1e-8, 100.0, 278.0, -278.0], np.float32)
    rng = np.random.default_rng(11)
    n = 6000
    O = vals[rng.integers(0, len(vals), (n, 3))]
    D = vals[rng.integers(0, len(vals), (n, 3))]
    # mostly ordinary origins / directions with one or two special components
    O[: n // 2] = rng.uniform(-300, 330, (n // 2, 3)).astype(np.float32)
    k = rng.integers(0, 3, n // 2)
    O[np.arange(n // 2), k] = vals[rng.integers(0, len(vals), n // 2)]
    # a -0 direction component beside positive ones (the world and the object reciprocal differ in the sign of an infinity there),
    # tiny or huge scales so that the other axes' distances overflow, origins outside the room on the zero axis
    m = np.arange(n // 2, n // 2 + 600)
    for i in m:
        ax = int(rng.integers(0, 3))
        D[i] = rng.choice(np.array([1e-40, 1e-8, 1.0, -1e-40], np.float32), 3)
        D[i, ax] = -0.0
        O[i] = rng.uniform(-300, 330, 3).astype(np.float32)
        O[i, ax] = rng.choice(np.array([-1e31, 1e31, -400.0, 400.0, -278.0, 0.0, -0.0], np.float32))
        if i % 4 == 0:
            with np.errstate(over="ignore"):
                O[i] *= np.float32(1e30)                                   # some components overflow: non-finite origins
    return O, D


def _tmax(n):
    rng = np.random.default_rng(12)
    tm = rng.uniform(0, 2000, n).astype(np.float32)
    tm[::5] = np.inf
    tm[1::7] = np.nan
    tm[2::11] = 0.0
    tm[3::13] = -0.0
    return tm


@pytest.mark.parametrize("scene_name", ["cornell_box", "cornell_mixed"])
def test_identity_scenes_take_the_one_ray_walk(api, scene_name):
    from path_tracer_amd import scenes
    sc = getattr(scenes, scene_name)(32, 32)
    assert _ident_tlas(api.Renderer(sc, 32, 32)) == 3
    assert _ident_tlas(api.Renderer(sc, 32, 32, flags=api.FLAG_GENERAL_WALK)) == 0


def test_rotated_instances_keep_the_general_walk(api):
    from path_tracer_amd import scenes
    assert _ident_tlas(api.Renderer(scenes.cornell_spheres(32, 32), 32, 32)) & 1 == 0


@pytest.mark.parametrize("scene_name", ["cornell_box", "cornell_mixed"])
def test_edge_rays_bit_equal_on_both_walks_and_vs_oracle(api, oracle_mod, scene_name):
    from path_tracer_amd import scenes
    sc = getattr(scenes, scene_name)(32, 32)
    fast = api.Renderer(sc, 32, 32)
    gen = api.Renderer(sc, 32, 32, flags=api.FLAG_GENERAL_WALK)
    o = oracle_mod.Oracle(sc)
    O, D = _edge_rays()
    tm = _tmax(len(O))
    for which in (0, 1):
        a = fast.trace_closest(O, D, which=which)
        b = gen.trace_closest(O, D, which=which)
        c = o.trace_closest(O, D, which=which)
        for k in ("inst", "prim", "t", "u", "v"):
            assert_bit_equal(a[k], b[k], f"{scene_name} tlas{which} closest.{k} ident vs general")
            assert_bit_equal(a[k], c[k], f"{scene_name} tlas{which} closest.{k} vs oracle")
        a = fast.trace_closest(O, D, tm, which=which)
        c = o.trace_closest(O, D, tm, which=which)
        for k in ("inst", "prim", "t"):
            assert_bit_equal(a[k], c[k], f"{scene_name} tlas{which} closest with t_max .{k} vs oracle")
        fa = fast.trace_any(O, D, tm, which=which)
        assert np.array_equal(fa, gen.trace_any(O, D, tm, which=which))
        assert np.array_equal(fa, o.trace_any(O, D, tm, which=which))


def test_one_rotated_instance_matches_oracle(api, oracle_mod):
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import affine_from_rotation_translation
    sc = scenes.cornell_box(32, 32)
    q = np.array([0.0, np.sin(0.3), 0.0, np.cos(0.3)], np.float32)            # (x, y, z, w): a turn about y
    tall = dataclasses.replace(sc.models[4], matrices=affine_from_rotation_translation(q, (0.0, 0.0, 0.0))[None].astype(np.float32))
    sc = dataclasses.replace(sc, models=[*sc.models[:4], tall, *sc.models[5:]])
    r = api.Renderer(sc, 32, 32)
    assert _ident_tlas(r) == 2                                                  # the lights TLAS still qualifies
    o = oracle_mod.Oracle(sc)
    rng = np.random.default_rng(5)
    n = 4000
    O = rng.uniform(-270, 270, (n, 3)).astype(np.float32)
    D = rng.normal(size=(n, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    E_O, E_D = _edge_rays()
    O = np.concatenate([O, E_O])
    D = np.concatenate([D, E_D])
    g = r.trace_closest(O, D)
    c = o.trace_closest(O, D)
    for k in ("inst", "prim", "t", "u", "v"):
        assert_bit_equal(g[k], c[k], f"rotated closest.{k}")
    tm = _tmax(len(O))
    assert np.array_equal(r.trace_any(O, D, tm), o.trace_any(O, D, tm))
    acc = r.render_samples(0, 2)
    assert_bit_equal(acc, api.Renderer(sc, 32, 32, flags=api.FLAG_GENERAL_WALK).render_samples(0, 2), "rotated frame")


def test_mixed_radiance_bit_equal_on_both_walks(api):
    from path_tracer_amd import scenes
    sc = scenes.cornell_mixed(48, 48)
    a = api.Renderer(sc, 48, 48, max_bounces=8).render_samples(0, 4)
    b = api.Renderer(sc, 48, 48, max_bounces=8, flags=api.FLAG_GENERAL_WALK).render_samples(0, 4)
    assert_bit_equal(a, b, "cornell_mixed per-sample radiance, one-ray vs general walk")
