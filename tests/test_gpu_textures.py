"""GPU: textured surface colour (pt_add_texture, pt_set_material_texture, pt_set_model_uvs), bit for bit.  The oracle knows nothing of textures,
so the expected values come three ways: the oracle's render of an untextured scene that the definition makes equivalent (texel corners); a
short composition from oracle pieces with the numpy restatement of the lookup in it (UVs that vary); the restatement alone (albedo guide,
unit hook).  tests/textures_common.py holds the restatement and the scenes."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from instances_common import apply, move, shifted
from textures_common import F, corner_scene, scene_surface_colour, varying_scene, world_instance_models

pytestmark = pytest.mark.gpu

W, H, DEPTH, SPP = 32, 24, 6, 2
LENS = (0.6, 9.0)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_CACHE = {}


def fma32(a, b, c):
    """f32::mul_add: a * b + c rounded ONCE to binary32.  The product of two binary32 values is exact in binary64; the sum is rounded to odd
    there (TwoSum gives the residual), which makes the final rounding to binary32 the correct one"""
    import math
    p = float(a) * float(b)
    c = float(c)
    s = p + c
    if math.isfinite(s):
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        if err != 0.0 and (np.float64(s).view(np.uint64) & np.uint64(1)) == 0:
            s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return F(s)


def _corner(oracle_mod, glass=True):
    """the two descriptions and the oracle's render of the untextured one, computed once"""
    key = "corner" if glass else "corner, no media"
    if key not in _CACHE:
        tex, plain = corner_scene(W, H, media=glass)
        orc = oracle_mod.Oracle(plain)
        samples = orc.render_samples(W, H, SPP + 2, max_bounces=DEPTH)
        frame = orc.render(W, H, SPP, max_bounces=DEPTH)
        _CACHE[key] = dict(tex=tex, plain=plain, orc=orc, samples=samples, frame=frame)
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


# ---- 1. texel corners: the whole integrator against the oracle's render of the equivalent untextured scene
@pytest.mark.parametrize("flags", [0, 2, 16], ids=["lds", "no_lds_scene", "general_walk"])
def test_texel_corners_render_as_the_untextured_equivalent(api, oracle_mod, flags):
    c = _corner(oracle_mod)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH, flags=flags)
    _check_render(r, c, f"flags {flags}")
    assert r.stats().lds_scene == (0 if flags == 2 else 1)
    # the loud texels are one texel away: the same scene with one model's corner moved is a different picture
    if flags == 0:
        r.set_model_uvs(1, np.broadcast_to(np.array([0.5, 0.0], F), (2, 3, 2)))
        r.rebuild()
        assert not np.array_equal(r.render_samples(0, 1), c["samples"][:1])


@pytest.mark.parametrize("flags", [0, 2], ids=["lds", "no_lds_scene"])
def test_texel_corners_without_media(api, oracle_mod, flags):
    """the same room without the glass boxes: no material carries a volume, so the shading passes are the TEX variants WITHOUT media (the
    room with the glass runs only those with), NEE on, against the oracle"""
    c = _corner(oracle_mod, glass=False)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH, flags=flags)
    _check_render(r, c, f"no media, flags {flags}")
    o, d, key, sample = _random_rays_box()
    got = r.integrate_rays(o, d, key, sample, draws_consumed=1)
    from test_gpu_rays import _oracle_rays
    want = _oracle_rays(c["orc"], o, d, key, sample, 1, DEPTH)
    assert_bit_equal(got[0], want[0], "no media, rays: radiance")


def _random_rays_box(n=500):
    from test_gpu_rays import _random_rays
    return _random_rays(np.array([-10, -10, -10, 10, 10, 10], F), n, 23)


def test_texel_corners_under_a_lens(api, oracle_mod):
    from test_gpu_lens import Expect
    tex, plain = corner_scene(W, H, lens=True)
    ex = Expect(oracle_mod, "corner", lens=LENS, w=W, h=H, depth=DEPTH, scene=plain)
    r = api.Renderer(tex, W, H, max_bounces=DEPTH)
    assert_bit_equal(r.render_samples(0, SPP), ex.samples(0, SPP), "lens: per-sample radiance")
    r.reset_accumulation()
    got = r.render(0, SPP)
    want = ex.frame(SPP)
    assert_bit_equal(got[0], want[0], "lens: accumulation"); assert_bit_equal(got[1], want[1], "lens: position")
    assert np.array_equal(got[2], want[2])


def test_texel_corners_through_caller_rays(api, oracle_mod):
    from test_gpu_rays import _oracle_rays, _random_rays
    c = _corner(oracle_mod)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    o, d, key, sample = _random_rays(np.array([-10, -10, -10, 10, 10, 10], F), 2000, 17)
    got = r.integrate_rays(o, d, key, sample, draws_consumed=1)
    want = _oracle_rays(c["orc"], o, d, key, sample, 1, DEPTH)
    assert_bit_equal(got[0], want[0], "rays: radiance"); assert_bit_equal(got[1], want[1], "rays: position")
    assert np.array_equal(got[2], want[2])


def test_texel_corners_adaptive_round(api, oracle_mod):
    from test_adaptive_host import criterion, luminance
    c = _corner(oracle_mod)
    s = c["samples"]
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    acc = (np.zeros_like(s[0]) + s[0]) + s[1]
    q = (np.zeros((H, W), F) + luminance(s[0]) * luminance(s[0])) + luminance(s[1]) * luminance(s[1])
    # a threshold the oracle's own two samples split the frame at: the median relative error of the noisy pixels
    m = luminance(acc) / F(2.0)
    rel = np.sqrt(np.maximum(q / F(2.0) - m * m, 0) / F(2.0)) / np.maximum(m, F(1e-3))
    crit = dict(rel_error=float(np.quantile(rel[rel > 0], 0.5)), abs_floor=0.0, min_samples=2, max_samples=0)
    assert r.render_adaptive(2, **crit) == W * H                                     # every pixel is below min_samples
    assert_bit_equal(r.read_frame()[0], acc, "adaptive round 1"); assert_bit_equal(r.read_moments(), q, "adaptive moments")
    want = criterion(acc, q, **crit)
    assert 0 < want.sum() < W * H, "the criterion should split the frame"
    assert r.render_adaptive(2, **crit) == int(want.sum())
    acc4 = (acc + s[2]) + s[3]
    assert_bit_equal(r.read_frame()[0], np.where(want[..., None], acc4, acc), "adaptive round 2")


def test_texel_corners_on_two_contexts(api, oracle_mod):
    c = _corner(oracle_mod)
    m = api.MultiRenderer(c["tex"], W, H, [0, 0], max_bounces=DEPTH, strip_rows=4)
    got = m.render(0, SPP)
    m.close()
    assert_bit_equal(got, c["frame"][0], "pt_multi over a duplicated device")


def test_texel_corners_after_a_move(api, oracle_mod):
    c = _corner(oracle_mod)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    r.render(0, 1)
    before = r.scene_info()
    tall = next(i for i, m in enumerate(c["tex"].models) if m.name == "tall")
    step = [(tall, shifted(c["tex"].models[tall].matrices, (-2.0, 0.5, 1.0)))]
    move(r, step)
    got = r.render_samples(0, SPP)
    after = r.scene_info()
    assert (after.uploads_patched, after.uploads_full, after.blas_builds) == (before.uploads_patched + 1, before.uploads_full, before.blas_builds)
    want = oracle_mod.Oracle(apply(c["plain"], step)).render_samples(W, H, SPP, max_bounces=DEPTH)
    assert_bit_equal(got, want, "moved textured scene")


# ---- 2. UVs that vary across a triangle: the sample composed from oracle pieces
def test_varying_uvs_compose_from_oracle_pieces(api, oracle_mod):
    """enable_nee = 0, max_bounces = 1: a sample is emitted * pw on a light, 0.006 * pw on a miss, else 0 after ONE Lambertian bounce whose
    colour is the restated surface colour"""
    from path_tracer_amd.scene_desc import Lambertian, Model, SceneDesc
    FRAC_1_PI = F(0.318309886183790671537767526745028724)
    desc = varying_scene(W, H)
    orc = oracle_mod.Oracle(desc)
    # material_eval looks at a material only: a white Lambertian lives in a little scene of its own
    white = Model.new(desc.models[1].positions, desc.models[1].normals, Lambertian.new((1.0, 1.0, 1.0)), None, "white")
    orc_w = oracle_mod.Oracle(SceneDesc.new([white], desc.camera))
    i_white = 0
    inst_model = world_instance_models(desc)
    emitted = np.array(desc.models[0].material.colour, F)
    r = api.Renderer(desc, W, H, max_bounces=1, enable_nee=False)
    got = r.render_samples(0, SPP)
    want = np.zeros((SPP, H, W, 4), F)
    n_textured = 0
    for s in range(SPP):
        for p in range(W * H):
            o, d = orc.primary_ray(W, H, p, s)
            h = orc.trace_closest(o[None], d[None])
            mi = int(inst_model[h["inst"][0]]) if h["inst"][0] != 0xFFFFFFFF else -1
            if mi < 0 or desc.models[mi].material.texture is None:
                want[s, p // W, p % W] = orc.integrate(o, d, p, s, 1, max_bounces=1, enable_nee=0)[0]
                continue
            n_textured += 1
            t, u, v, prim = h["t"][0], h["u"][0], h["v"][0], h["prim"][0]
            nrm, front = h["normal"][0], int(h["front"][0])
            ev = orc_w.material_eval(i_white, d, nrm, front, p, s, draws_consumed=1)            # wo xyz, bsdf rgb, pdf, weakening, draws
            wo, pdf, weak = ev[0:3], ev[6], ev[7]
            colour = scene_surface_colour(desc, inst_model, [h["inst"][0]], [prim], [u], [v])[0]
            bsdf = colour * FRAC_1_PI
            pw = (weak * bsdf) / pdf
            at = np.array([fma32(d[k], t, o[k]) for k in range(3)], F)                        # r.at(t): mul_add per component
            h2 = orc.trace_closest(at[None], wo[None])
            if h2["inst"][0] == 0xFFFFFFFF:
                rad = F(0.006) * pw
            elif desc.models[int(inst_model[h2["inst"][0]])].material.kind == 1:
                rad = np.array([fma32(emitted[k], pw[k], 0.0) for k in range(3)], F)          # emitted.mul_add(pw, 0)
            else:
                rad = np.zeros(3, F)
            if pdf < 0:                                                                       # MIN_PDF = 0: the path ends at the first hit
                rad = np.zeros(3, F)
            if not np.isfinite(rad).all():                                                    # integrator.rs:272
                rad = np.zeros(3, F)
            assert float(np.sqrt((rad.astype(np.float64) ** 2).sum())) < 99.0                # below the 100 clamp: it never has to be restated
            want[s, p // W, p % W] = (rad[0], rad[1], rad[2], 1.0)
    assert n_textured > W * H * SPP // 3
    assert_bit_equal(got, want, "composed samples")


# ---- 3. the albedo guide
def test_albedo_guide_is_the_surface_colour_at_the_first_hit(api, oracle_mod):
    desc = varying_scene(W, H)
    orc = oracle_mod.Oracle(desc)
    r = api.Renderer(desc, W, H, max_bounces=DEPTH)
    plain = api.Renderer(desc, W, H, max_bounces=DEPTH)
    inst_model = world_instance_models(desc)
    k = 3
    r.render_guides(k)
    o = np.zeros((W * H, 3), F); d = np.zeros((W * H, 3), F)
    for p in range(W * H):
        o[p], d[p] = orc.primary_ray(W, H, p, k)
    h = orc.trace_closest(o, d)
    hit = h["inst"] != 0xFFFFFFFF
    want = np.zeros((W * H, 3), F)
    want[hit] = scene_surface_colour(desc, inst_model, h["inst"][hit], h["prim"][hit], h["u"][hit], h["v"][hit])
    models = inst_model[h["inst"][hit]]
    assert (~hit).any() and (models == 0).any() and (models == 1).any() and (models == 3).any(), "misses, the light, textured and untextured hits"
    assert_bit_equal(r.read_guide_albedo().reshape(-1, 3), want, "albedo guide")
    pos, nrm, model = r.read_guides()
    inst = r.read_guide_instances()
    # the other four guides are what a context that never heard of textures keeps
    plain.set_material_texture(1, -1); plain.rebuild()
    plain.render_guides(k)
    ppos, pnrm, pmodel = plain.read_guides()
    assert_bit_equal(pos, ppos, "position guide"); assert_bit_equal(nrm, pnrm, "normal guide")
    assert np.array_equal(model, pmodel) and np.array_equal(inst, plain.read_guide_instances())
    assert np.array_equal(inst.reshape(-1)[hit], h["inst"][hit]) and (inst.reshape(-1)[~hit] == 0xFFFFFFFF).all()
    untouched = np.ones(W * H, bool)
    untouched[hit] = (models != 1) & (models != 2)
    assert_bit_equal(plain.read_guide_albedo().reshape(-1, 3)[untouched], want[untouched], "albedo away from the textured models")


# ---- 4. the unit hook on the device
def test_surface_colour_on_the_device_is_the_host_evaluation(api):
    from test_textures_host import _desc, _queries
    desc = _desc()
    r = api.Renderer(desc, 16, 16)
    inst, prim, u, v = _queries(desc)
    host = r.surface_colour(inst, prim, u, v)
    assert_bit_equal(r.surface_colour(inst, prim, u, v, on_device=True), host, "surface colour, device")
    plain = api.Renderer(_desc(textured=False), 16, 16)                                      # no texture view at all on the device
    assert_bit_equal(plain.surface_colour(inst, prim, u, v, on_device=True), plain.surface_colour(inst, prim, u, v), "untextured scene")


# ---- 5. the C++ driver
def test_headless_checker_writes_what_the_python_route_presents(api, tmp_path):
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc, Texture
    from test_gpu_post import _read_png
    n, w, h = 8, 48, 32
    exe = B.build_host_driver()
    out = tmp_path / "checker.png"
    run = subprocess.run([exe, "--width", str(w), "--height", str(h), "--bounces", str(DEPTH), "--render", "0", "3", "--checker", str(n), "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    tex = Texture.new(np.repeat(np.where((i + j) & 1, F(0.2), F(1.0))[..., None], 3, axis=2))
    src = scenes.cornell_models()
    models = [Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material.textured(tex) if m.name == "cb_main" else m.material)
              for m in src]
    assert [m.name for m in src][1] == "cb_main"
    r = api.Renderer(SceneDesc.new(models, scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    p, _ = r.model_vertices(1)
    xz = p[:, :, [0, 2]]
    lo, hi = xz.min(axis=(0, 1)), xz.max(axis=(0, 1))
    r.set_model_uvs(1, (xz - lo) / (hi - lo))
    r.rebuild()
    r.render(0, 3)
    assert np.array_equal(_read_png(out), r.present_rgb8().reshape(h, w, 3))
    plain = api.Renderer(SceneDesc.new([Model.from_obj(m.obj_path, s.material) for m, s in zip(models, src)], scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    plain.render(0, 3)
    assert not np.array_equal(plain.present_rgb8(), r.present_rgb8())
