"""GPU: emission textures (pt_set_material_emission_texture), bit for bit where the definition allows it.  The oracle knows nothing of textures, so
the expected values come from: the oracle's render of an untextured scene that the definition makes equivalent (lamps at texel corners); a
short composition from oracle pieces with the numpy restatement of the lookup in it (UVs that vary over a lamp, NEE off); a zero / nonzero
prediction of both direct-light estimates (NEE on, the (triangle, u, v) each of them reads); and, for what bit-exactness cannot show, the
agreement of the NEE and the plain estimator in the mean.  tests/emission_common.py holds the restatement and the scenes."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from emission_common import (F, MIRROR, N_LAMPS, dim_scene, emission_corner_scene, fma32, plumbing_scene, scene_colour, varying_light_scene,
                             world_instance_models)
from instances_common import apply, move, shifted

pytestmark = pytest.mark.gpu

W, H, DEPTH, SPP = 32, 24, 6, 2
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_CACHE = {}


def _corner(oracle_mod, glass=True, nee=True):
    """the descriptions and the oracle's renders of the untextured one, computed once per (media, NEE)"""
    key = (glass, nee)
    if key not in _CACHE:
        tex, plain = emission_corner_scene(W, H, media=glass)
        only, _ = emission_corner_scene(W, H, media=glass, wall_textures=False)
        orc = oracle_mod.Oracle(plain)
        kw = dict(max_bounces=DEPTH, enable_nee=int(nee))
        _CACHE[key] = dict(tex=tex, plain=plain, only=only, orc=orc, samples=orc.render_samples(W, H, SPP, **kw), frame=orc.render(W, H, SPP, **kw))
    return _CACHE[key]


def _check_render(r, c, what):
    got = r.render_samples(0, SPP)
    assert_bit_equal(got, c["samples"][:SPP], what + ": per-sample radiance")
    r.reset_accumulation(); r.reset_stats()
    acc, pos, idb = r.render(0, SPP)
    oacc, opos, oid, octr = c["frame"]
    assert_bit_equal(acc, oacc, what + ": accumulation"); assert_bit_equal(pos, opos, what + ": position")
    assert np.array_equal(idb, oid), what + ": id history"
    st = r.stats()
    assert (st.rays_closest, st.rays_any, st.rays_light_closest) == (int(octr[0]), int(octr[1]), int(octr[2])), what + ": ray tallies"


def _first_hits(orc, sample=0):
    o = np.zeros((W * H, 3), F); d = np.zeros((W * H, 3), F)
    for p in range(W * H):
        o[p], d[p] = orc.primary_ray(W, H, p, sample)
    return o, d, orc.trace_closest(o, d)


# ---- 1. lamps at texel corners: the whole integrator against the oracle's render of the equivalent untextured scene
@pytest.mark.parametrize("glass", [True, False], ids=["media", "no_media"])
@pytest.mark.parametrize("nee", [True, False], ids=["nee", "no_nee"])
@pytest.mark.parametrize("flags", [0, 2, 16], ids=["lds", "no_lds_scene", "general_walk"])
def test_lamps_at_texel_corners_render_as_the_untextured_equivalent(api, oracle_mod, flags, nee, glass):
    c = _corner(oracle_mod, glass, nee)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH, flags=flags, enable_nee=nee)
    _check_render(r, c, f"flags {flags}, nee {nee}, media {glass}")
    assert r.stats().lds_scene == (0 if flags == 2 else 1)


def test_the_scene_shows_its_lamps_and_a_loud_texel_changes_it(api, oracle_mod):
    c = _corner(oracle_mod)
    inst_model = world_instance_models(c["plain"])
    o, d, h = _first_hits(c["orc"])
    hit = h["inst"] != MISS
    models = inst_model[h["inst"][hit]]
    assert (models < N_LAMPS).sum() >= 10, "some pixels see a textured lamp directly"
    # ... and the mirror shows one: reflect the camera ray off it (utility.rs reflect: d - 2 (d . n) n; exactness does not matter for a count)
    on_mirror = np.nonzero(hit)[0][models == MIRROR]
    assert len(on_mirror) > 0
    dm, nm = d[on_mirror].astype(np.float64), h["normal"][on_mirror].astype(np.float64)
    wo = dm - 2.0 * (dm * nm).sum(1)[:, None] * nm
    at = o[on_mirror] + d[on_mirror] * h["t"][on_mirror][:, None]
    h2 = c["orc"].trace_closest((at + 1e-3 * wo).astype(F), wo.astype(F))
    seen = h2["inst"] != MISS
    assert (inst_model[h2["inst"][seen]] < N_LAMPS).any(), "the mirror block reflects a textured lamp"
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    assert_bit_equal(r.render_samples(0, 1), c["samples"][:1], "before the edit")
    r.set_model_uvs(0, np.broadcast_to(np.array([0.25, 0.0], F), (2, 3, 2)))       # the wall lamp's corner moved onto a loud texel
    r.rebuild()
    assert not np.array_equal(r.render_samples(0, 1), c["samples"][:1])


@pytest.mark.parametrize("glass", [True, False], ids=["media", "no_media"])
def test_an_emission_texture_as_the_only_texture(api, oracle_mod, glass):
    c = _corner(oracle_mod, glass)
    assert all(m.material.texture is None for m in c["only"].models)
    r = api.Renderer(c["only"], W, H, max_bounces=DEPTH)
    _check_render(r, c, f"emission texture only, media {glass}")


# ---- 2. the same scene through other routes
def test_corner_lamps_through_caller_rays(api, oracle_mod):
    from test_gpu_rays import _oracle_rays, _random_rays
    c = _corner(oracle_mod)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    o, d, key, sample = _random_rays(np.array([-10, -10, -10, 10, 10, 10], F), 2000, 29)
    got = r.integrate_rays(o, d, key, sample, draws_consumed=1)
    want = _oracle_rays(c["orc"], o, d, key, sample, 1, DEPTH)
    assert_bit_equal(got[0], want[0], "rays: radiance"); assert_bit_equal(got[1], want[1], "rays: position")
    assert np.array_equal(got[2], want[2])


def test_corner_lamps_on_two_contexts(api, oracle_mod):
    c = _corner(oracle_mod)
    m = api.MultiRenderer(c["tex"], W, H, [0, 0], max_bounces=DEPTH, strip_rows=4)
    got = m.render(0, SPP)
    m.close()
    assert_bit_equal(got, c["frame"][0], "pt_multi over a duplicated device")


def test_corner_lamps_after_moving_one(api, oracle_mod):
    c = _corner(oracle_mod)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    r.render(0, 1)
    before = r.scene_info()
    lamp = next(i for i, m in enumerate(c["tex"].models) if m.name == "lamp_turned")
    step = [(lamp, shifted(c["tex"].models[lamp].matrices, (-3.0, -1.5, -2.0)))]
    move(r, step)
    got = r.render_samples(0, SPP)
    after = r.scene_info()
    assert (after.uploads_patched, after.uploads_full, after.blas_builds) == (before.uploads_patched + 1, before.uploads_full, before.blas_builds)
    want = oracle_mod.Oracle(apply(c["plain"], step)).render_samples(W, H, SPP, max_bounces=DEPTH)
    assert_bit_equal(got, want, "moved lamp")


# ---- 3. NEE off, UVs that vary over the lamp: the sample composed from oracle pieces
def test_varying_lamp_uvs_compose_from_oracle_pieces(api, oracle_mod):
    """enable_nee = 0, max_bounces = 1: a sample is emitted on a lamp seen directly, 0.006 on a miss, else after ONE bounce emitted * pw on the
    lamp, 0.006 * pw on a miss and 0 elsewhere; emitted is the restated surface colour at the light hit"""
    desc = varying_light_scene(W, H)
    orc = oracle_mod.Oracle(desc)
    inst_model = world_instance_models(desc)
    r = api.Renderer(desc, W, H, max_bounces=1, enable_nee=False)
    got = r.render_samples(0, SPP)
    want = np.zeros((SPP, H, W, 4), F)
    n_direct = n_bounced = 0
    for s in range(SPP):
        for p in range(W * H):
            o, d = orc.primary_ray(W, H, p, s)
            h = orc.trace_closest(o[None], d[None])
            if h["inst"][0] == MISS:
                want[s, p // W, p % W] = orc.integrate(o, d, p, s, 1, max_bounces=1, enable_nee=0)[0]
                continue
            mi = int(inst_model[h["inst"][0]])
            if mi == 0:                                                                       # the lamp, seen directly: emitted.mul_add(1, 0)
                rad = scene_colour(desc, inst_model, [h["inst"][0]], [h["prim"][0]], [h["u"][0]], [h["v"][0]])[0]
                n_direct += 1
            else:
                ev = orc.material_eval(mi, d, h["normal"][0], int(h["front"][0]), p, s, draws_consumed=1)   # wo xyz, bsdf rgb, pdf, weakening, draws
                wo, bsdf, pdf, weak = ev[0:3], ev[3:6], ev[6], ev[7]
                pw = (weak * bsdf) / pdf
                at = np.array([fma32(d[k], h["t"][0], o[k]) for k in range(3)], F)            # r.at(t): mul_add per component
                h2 = orc.trace_closest(at[None], wo[None])
                if h2["inst"][0] == MISS:
                    rad = F(0.006) * pw
                elif int(inst_model[h2["inst"][0]]) == 0:
                    e = scene_colour(desc, inst_model, [h2["inst"][0]], [h2["prim"][0]], [h2["u"][0]], [h2["v"][0]])[0]
                    rad = np.array([fma32(e[k], pw[k], 0.0) for k in range(3)], F)            # emitted.mul_add(pw, 0)
                    n_bounced += mi == 1                                                      # ... after a Lambertian bounce off the floor
                else:
                    rad = np.zeros(3, F)
                if pdf < 0 or not np.isfinite(rad).all():                                     # MIN_PDF = 0; integrator.rs:272
                    rad = np.zeros(3, F)
            assert float(np.sqrt((rad.astype(np.float64) ** 2).sum())) < 99.0                # below the 100 clamp: it never has to be restated
            want[s, p // W, p % W] = (rad[0], rad[1], rad[2], 1.0)
    assert n_direct > 100 and n_bounced > 10, (n_direct, n_bounced)
    assert_bit_equal(got, want, "composed samples")


# ---- 4. NEE on: the (triangle, u, v) each direct-light estimate reads
def test_both_estimates_read_the_texture_where_they_should(api, oracle_mod):
    """max_bounces = 0 over a white floor under a lamp of texels 0 and 8: a sample is explicit + BSDF estimate, exactly zero when both read
    black and nonzero otherwise (tests/test_emission_textures_host.py checks that each class is large and the excluded one small)"""
    from test_emission_textures_host import plumbing_classes
    pred = plumbing_classes(api, oracle_mod).reshape(SPP, H, W)
    r = api.Renderer(plumbing_scene(W, H), W, H, max_bounces=0, enable_nee=True)
    got = r.render_samples(0, SPP)
    zero = pred == 0
    lit = pred == 1
    print("plumbing: predicted zero", int(zero.sum()), "nonzero", int(lit.sum()), "excluded", int((pred == 2).sum()))
    assert zero.sum() >= 0.2 * pred.size and lit.sum() >= 0.2 * pred.size and (pred == 2).sum() <= 0.01 * pred.size
    assert_bit_equal(got[zero], np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0], F), got[zero].shape), "predicted-zero samples")
    assert (got[lit][:, :3] != 0).any(axis=1).all(), f"{int((~(got[lit][:, :3] != 0).any(axis=1)).sum())} predicted-nonzero samples are black"
    assert (got[..., 3] == 1).all()


# ---- 5. unbiasedness of the definition: NEE with the one-point weights and MIS against plain path tracing, in the mean
def test_nee_and_plain_path_tracing_agree_in_the_mean(api):
    n = 256
    lum = {}
    for nee in (True, False):
        r = api.Renderer(dim_scene(W, H), W, H, max_bounces=DEPTH, enable_nee=nee)
        s = r.render_samples(0, n).astype(np.float64)
        assert (s[..., 3] == 1).all()
        assert np.sqrt((s[..., :3] ** 2).sum(-1)).max() < 99.0, "the clamp at 100 never acts"
        lum[nee] = 0.2126 * s[..., 0] + 0.7152 * s[..., 1] + 0.0722 * s[..., 2]               # [n, H, W]
    # the image mean is the mean of W * H independent per-pixel means: its variance is the mean per-pixel sample variance over N = n * W * H
    N = n * W * H
    mean = {k: v.mean() for k, v in lum.items()}
    var = {k: v.var(axis=0, ddof=1).mean() for k, v in lum.items()}
    sigma = np.sqrt(var[True] / N + var[False] / N)
    diff = mean[True] - mean[False]
    print(f"mean luminance NEE {mean[True]:.6f}, plain {mean[False]:.6f}, diff {diff:+.6f}, sigma {sigma:.6f} ({diff / sigma:+.2f} sigma)")
    assert mean[False] > 0.05 and var[True] < var[False]
    assert abs(diff) <= 4.0 * sigma


# ---- 6. guides and the unit hook
def test_guides_carry_the_textured_emitted_colour(api, oracle_mod):
    desc = varying_light_scene(W, H)
    orc = oracle_mod.Oracle(desc)
    r = api.Renderer(desc, W, H, max_bounces=DEPTH)
    inst_model = world_instance_models(desc)
    k = 3
    o, d, h = _first_hits(orc, k)
    hit = h["inst"] != MISS
    want = np.zeros((W * H, 3), F)
    want[hit] = scene_colour(desc, inst_model, h["inst"][hit], h["prim"][hit], h["u"][hit], h["v"][hit])
    first = np.full(W * H, -1); first[hit] = inst_model[h["inst"][hit]]
    assert (first == 0).sum() > 50 and (first == 2).any() and (~hit).any()
    r.render_guides(k)
    assert_bit_equal(r.read_guide_albedo().reshape(-1, 3), want, "albedo guide")
    assert len(np.unique(want[first == 0], axis=0)) > 50, "the lamp's colour varies over the picture"
    # followed through the mirror (colour 1, 1, 1): albedo = c_0 * c_1 = 1 * the emitted colour where the reflection ends on the lamp
    r.render_guides(k, follow=1)
    got = r.read_guide_albedo().reshape(-1, 3)
    hops = r.read_guide_hops().reshape(-1)
    assert_bit_equal(got[first != 2], want[first != 2], "followed guides away from the mirror")
    on = np.nonzero(first == 2)[0]
    fd = r.guide_follow_dir(2, d[on], h["normal"][on], h["front"][on])
    assert (fd[:, 3] == 1).all() and (hops[on] == 1).all()
    at = np.array([[fma32(d[i][c], h["t"][i], o[i][c]) for c in range(3)] for i in on], F)
    h2 = orc.trace_closest(at, fd[:, :3])
    ends = h2["inst"] != MISS
    c1 = np.zeros((len(on), 3), F)
    c1[ends] = scene_colour(desc, inst_model, h2["inst"][ends], h2["prim"][ends], h2["u"][ends], h2["v"][ends])
    assert (inst_model[h2["inst"][ends]] == 0).sum() >= 3, "the mirror shows the lamp"
    assert_bit_equal(got[on], F(1.0) * c1, "followed guides through the mirror")


def test_surface_colour_on_the_device_is_the_host_evaluation(api):
    desc = varying_light_scene(W, H)
    r = api.Renderer(desc, W, H)
    rng = np.random.default_rng(4)
    n = 3000
    inst = rng.integers(0, 3, n).astype(np.uint32)
    prim = (rng.integers(0, 1 << 20, n) % np.array([2, 2, 12])[inst]).astype(np.uint32)
    u = rng.uniform(0.0, 1.0, n).astype(F)
    v = (rng.uniform(0.0, 1.0, n).astype(F) * (F(1.0) - u)).astype(F)
    host = r.surface_colour(inst, prim, u, v)
    assert_bit_equal(host, scene_colour(desc, world_instance_models(desc), inst, prim, u, v), "surface colour, host")
    assert_bit_equal(r.surface_colour(inst, prim, u, v, on_device=True), host, "surface colour, device")


# ---- 7. the C++ driver
def test_headless_emission_checker_writes_what_the_python_route_presents(api, tmp_path):
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc, Texture
    from test_gpu_post import _read_png
    n, w, h = 8, 48, 32
    exe = B.build_host_driver()
    out = tmp_path / "emission.png"
    run = subprocess.run([exe, "--width", str(w), "--height", str(h), "--bounces", str(DEPTH), "--render", "0", "3", "--emission-checker", str(n), "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    tex = Texture.new(np.repeat(np.where((i + j) & 1, F(0.2), F(1.0))[..., None], 3, axis=2))
    src = scenes.cornell_models()
    assert [m.name for m in src][0] == "cb_light"
    models = [Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material.emission_textured(tex) if m.name == "cb_light" else m.material)
              for m in src]
    r = api.Renderer(SceneDesc.new(models, scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    p, _ = r.model_vertices(0)
    xz = p[:, :, [0, 2]]
    lo, hi = xz.min(axis=(0, 1)), xz.max(axis=(0, 1))
    r.set_model_uvs(0, (xz - lo) / (hi - lo))
    r.rebuild()
    r.render(0, 3)
    assert np.array_equal(_read_png(out), r.present_rgb8().reshape(h, w, 3))
    plain = api.Renderer(SceneDesc.new([Model.from_obj(m.obj_path, s.material) for m, s in zip(models, src)], scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    plain.render(0, 3)
    assert not np.array_equal(plain.present_rgb8(), r.present_rgb8())
