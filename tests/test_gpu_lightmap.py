"""GPU: lightmaps (pt_bake_lightmap, pt_lightmap_texels on the device, pt_lightmap_dilate), bit for bit.  Expected values are the numpy
restatement of tests/lightmap_common.py for the texel table, the rays and the dilation, and the oracle's integrator walked from those rays with
the same stream keys (Oracle.integrate), folded in numpy in sample order."""
import os
import subprocess

import numpy as np
import pytest

import lightmap_common as LC
from conftest import ROOT, assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
W, H, DEPTH = 48, 32, 6
NO_LDS_SCENE = 2


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _renderer(api, sc, flags=0, **kw):
    return api.Renderer(sc, W, H, max_bounces=DEPTH, flags=flags, **kw)


# ---- 1. the texel table on the device
@pytest.mark.parametrize("name", LC.TEXEL_CASES)
def test_device_texel_table_equals_the_host(api, name):
    case = LC.texel_case(name)
    host = LC.query_texels(api, case, on_device=False)
    LC.check_case_is_meaningful(name, host)
    dev = LC.query_texels(api, case, on_device=True)
    assert np.array_equal(dev[0], host[0]), f"{name}: owners"
    for d, h, what in zip(dev[1:], host[1:], ("uv", "position", "normal")):
        assert_bit_equal(d, h, f"{name}: {what}")


# ---- 2. the bake against the oracle
_SCENES = {}
_EXPECT = {}


def _scene(which):
    """(scene, model, instance, oracle's scene) of a bake case; the oracle reads the same models (UVs mean nothing to it)"""
    if which not in _SCENES:
        if which == "instanced":
            sc = LC.instanced_atlas_scene(W, H)
            _SCENES[which] = (sc, LC.INSTANCED_MODEL, LC.INSTANCED_INSTANCE)
        else:
            sc, model = LC.cornell_atlas_scene(which, W, H)
            _SCENES[which] = (sc, model, 0)
    return _SCENES[which]


def _expected(O, which, w, h, n, first=0, key_base=0, bias=0.0):
    """(texel table, covered texel indices, the bake's rays, their radiance by the oracle), computed once per case"""
    key = (which, w, h, n, first, key_base, bias)
    if key not in _EXPECT:
        sc, model, instance = _scene(which)
        m = sc.models[model]
        table = LC.texels(m.positions, m.normals, m.uvs, m.matrices[instance], w, h)
        k, o, d, keys, samples = LC.bake_rays(O, table, n, first, key_base, bias)
        if ("oracle", which) not in _SCENES:
            _SCENES[("oracle", which)] = O.Oracle(sc)
        orc = _SCENES[("oracle", which)]
        rad = np.array([orc.integrate(o[i], d[i], int(keys[i]), int(samples[i]), 1, max_bounces=DEPTH)[0] for i in range(len(keys))], F)
        _EXPECT[key] = (table, k, (o, d, keys, samples), rad)
    return _EXPECT[key]


def _check_bake(api, O, which, w, h, n, flags=0, start_seed=None, **kw):
    sc, model, instance = _scene(which)
    table, k, _, rad = _expected(O, which, w, h, n, **kw)
    start = np.zeros((h, w, 3), F) if start_seed is None else np.random.default_rng(start_seed).uniform(-1, 1, (h, w, 3)).astype(F)
    want = LC.fold(start, k, rad, n)
    r = _renderer(api, sc, flags)
    before = r.stats().paths
    sums, cov = r.bake_lightmap(model, instance, w, h, n, first_sample=kw.get("first", 0), key_base=kw.get("key_base", 0), bias=kw.get("bias", 0.0),
                                sums=start.copy())
    what = f"{which} {w}x{h} flags {flags} {kw}"
    assert np.array_equal(cov, (table[0] != LC.MISS).astype(np.uint8)), what + ": coverage"
    assert_bit_equal(sums, want, what + ": sums")
    assert_bit_equal(sums[cov == 0], start[cov == 0], what + ": uncovered texels")
    assert np.abs(sums[cov == 1] - start[cov == 1]).max() > 0
    assert r.stats().paths - before == len(k) * n
    assert r.stats().lds_scene == (0 if flags & NO_LDS_SCENE else 1)
    return r, sums


@pytest.mark.parametrize("flags", [0, NO_LDS_SCENE], ids=["lds", "global"])
def test_bake_against_the_oracle(api, oracle_mod, flags):
    """cb_box_short under the atlas, 12 x 8, 8 samples: 80 covered texels, 640 rays; the sums start from random values, so an uncovered texel
    that was written shows"""
    _, k, _, rad = _expected(oracle_mod, "cb_box_short", 12, 8, 8, key_base=1000, bias=0.25)
    assert len(k) == 80 and len(rad) == 640 and (rad[:, :3] > 0).any()
    _check_bake(api, oracle_mod, "cb_box_short", 12, 8, 8, flags=flags, start_seed=2, key_base=1000, bias=0.25)


def test_bake_without_bias(api, oracle_mod):
    _check_bake(api, oracle_mod, "cb_box_short", 12, 8, 8, key_base=1000, bias=0.0)


def test_bake_continues_late_samples_and_high_keys(api, oracle_mod):
    _check_bake(api, oracle_mod, "cb_box_short", 12, 8, 8, start_seed=3, first=500, key_base=0xFFFFFF00, bias=0.25)


def test_split_bakes_batch_cuts_and_ray_order_do_not_matter(api, oracle_mod):
    sc, model, instance = _scene("cb_box_short")
    table, k, (o, d, keys, samples), _ = _expected(oracle_mod, "cb_box_short", 12, 8, 8, key_base=1000, bias=0.25)
    r, whole = _check_bake(api, oracle_mod, "cb_box_short", 12, 8, 8, key_base=1000, bias=0.25)
    part, _ = r.bake_lightmap(model, instance, 12, 8, 3, key_base=1000, bias=0.25)
    part, _ = r.bake_lightmap(model, instance, 12, 8, 5, first_sample=3, key_base=1000, bias=0.25, sums=part)
    assert_bit_equal(part, whole, "bake(0, 3) then bake(3, 5)")
    # wavefront batches of 2 * 80 rays, three to a ray table: a texel's 8 samples straddle both cuts
    cut = _renderer(api, sc, batch_spp=2)
    assert_bit_equal(cut.bake_lightmap(model, instance, 12, 8, 8, key_base=1000, bias=0.25)[0], whole, "cut into batches")
    # the restated rays through integrate_rays in a shuffled order
    order = np.random.default_rng(4).permutation(len(keys))
    rad = np.zeros((len(keys), 4), F)
    rad[order] = r.integrate_rays(o[order], d[order], keys[order], samples[order])[0]
    assert_bit_equal(LC.fold(np.zeros((8, 12, 3), F), k, rad, 8), whole, "integrate_rays on the restated rays")


def test_small_map_and_general_rigid_instance(api, oracle_mod):
    _check_bake(api, oracle_mod, "cb_box_short", 5, 3, 8, key_base=7, bias=0.25)
    _check_bake(api, oracle_mod, "instanced", 12, 8, 4, key_base=7, bias=0.25)


def test_a_map_without_a_covered_texel_is_fine(api):
    sc = LC.quad_scene(LC.QUAD_UV + F(3.0), light=True)
    r = _renderer(api, sc)
    sums, cov = r.bake_lightmap(0, 0, 4, 4, 2, sums=np.full((4, 4, 3), 5, F))
    assert not cov.any() and (sums == 5).all() and r.stats().paths == 0


# ---- 3. independent of both restatements
def test_constant_environment_gives_one(api):
    """one quad under an environment of radiance 1, NEE off: every ray leaves the scene (they start 0.25 above the quad), so every texel's
    mean is 1; 1e-5 bounds the rounding of the environment's bilinear weights"""
    r = _renderer(api, LC.quad_scene(), enable_nee=False)
    r.set_environment(np.ones((4, 8, 3), F))
    sums, cov = r.bake_lightmap(0, 0, 8, 8, 16, bias=0.25)
    assert (cov == 1).all()
    assert np.abs(sums / F(16) - 1.0).max() < 1e-5, np.abs(sums / F(16) - 1.0).max()


# ---- 4. dilation
def _box_map():
    sc, model = LC.cornell_atlas_scene()
    cov = (LC.coverage(sc.models[model].uvs, 16, 16)[0] != LC.MISS).astype(np.uint8)
    rgb = np.random.default_rng(8).uniform(0, 4, (16, 16, 3)).astype(F)
    return rgb, cov


@pytest.mark.parametrize("passes", [1, 3])
def test_dilation_is_the_definition(api, passes):
    r = _renderer(api, LC.quad_scene())
    rgb, cov = _box_map()
    want_rgb, want_cov = LC.dilate(rgb, cov, passes)
    assert (want_cov == 2).sum() > 0 and (passes == 3 or (want_cov == 0).sum() > 0)
    got_rgb, got_cov = r.dilate_lightmap(rgb, cov, passes)
    assert np.array_equal(got_cov, want_cov)
    assert_bit_equal(got_rgb, want_rgb, f"{passes} passes")


def test_dilation_leaves_full_and_empty_maps_alone(api):
    r = _renderer(api, LC.quad_scene())
    rgb, _ = _box_map()
    for value in (1, 0):
        cov = np.full((16, 16), value, np.uint8)
        got_rgb, got_cov = r.dilate_lightmap(rgb, cov, 2)
        assert np.array_equal(got_cov, cov)
        assert_bit_equal(got_rgb, rgb, f"coverage all {value}")


# ---- 5. the C++ surface
def test_headless_bakes_a_lightmap(api, tmp_path):
    """examples/headless --bake-lightmap 16 16 8 2 out.txt parses back to the Python surface's bake and dilation under the same UVs"""
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, BOUNCES = 48, 32, 4
    exe = B.build_host_driver()
    out_txt = tmp_path / "lightmap.txt"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES), "--bake-lightmap", "16", "16", "8", "2",
                          str(out_txt)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    rows = [line.split() for line in out_txt.read_text().splitlines()]
    assert len(rows) == 256 and all(len(v) == 4 for v in rows)
    got_cov = np.array([int(v[0]) for v in rows], np.uint8).reshape(16, 16)
    got = np.array([[float.fromhex(x) for x in v[1:]] for v in rows], np.float64)
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    p = r.model_vertices(1)[0].reshape(-1, 3)[:, [0, 2]]
    lo, hi = p.min(0), p.max(0)
    r.set_model_uvs(1, ((p - lo) / (hi - lo)).astype(F).reshape(-1, 3, 2))
    r.rebuild()
    sums, cov = r.bake_lightmap(1, 0, 16, 16, 8, bias=0.25)
    assert (cov == 1).all()                  # floor and ceiling overlap over the whole square; the floor's triangles come first
    want, want_cov = r.dilate_lightmap(sums, cov, 2)
    assert np.array_equal(got_cov, want_cov)
    assert_bit_equal(got.astype(F).reshape(16, 16, 3), want, "headless --bake-lightmap")
    assert np.array_equal(got, got.astype(F).astype(np.float64)) and (want > 0).any()
