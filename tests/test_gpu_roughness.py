"""GPU: roughness maps (pt_set_material_roughness_texture), bit for bit.  The oracle knows nothing of textures, so the expected values come
three ways: the oracle's render of an untextured scene that the definition makes equivalent (texel corners, constant maps); a composition
from oracle pieces in which every hit is shaded by an oracle whose material has the hit's restated roughness (a map that varies); the numpy
restatement alone (the unit hook, the baked view).  tests/roughness_common.py holds the restatement and the scenes.  Every render here fails on
a library that ignores the map: no value of a map is the roughness of the material under it."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import roughness_common as RC
from conftest import ROOT, assert_bit_equal
from roughness_common import F
from textures_common import world_instance_models

pytestmark = pytest.mark.gpu

W, H, DEPTH, SPP = 32, 24, 4, 3          # the variant census's shapes
QW, QH, QSPP = 8, 8, 2                   # the normal-map composition's (max_bounces = 1)
LENS = (0.6, 9.0)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_CACHE = {}


def _room(oracle_mod, key, make):
    """(the mapped description, its untextured equivalent, the oracle's render of the equivalent), computed once per key"""
    if key not in _CACHE:
        mapped, plain = make()
        orc = oracle_mod.Oracle(plain)
        _CACHE[key] = dict(tex=mapped, plain=plain, orc=orc, samples=orc.render_samples(W, H, SPP + 1, max_bounces=DEPTH),
                           frame=orc.render(W, H, SPP, max_bounces=DEPTH))
    return _CACHE[key]


def _corner(oracle_mod, media=True):
    return _room(oracle_mod, ("corner", media), lambda: RC.corner_room(W, H, media=media))


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
@pytest.mark.parametrize("media", [True, False], ids=["media", "no_media"])
def test_texel_corners_render_as_the_untextured_equivalent(api, oracle_mod, media, flags):
    c = _corner(oracle_mod, media)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH, flags=flags)
    _check_render(r, c, f"media {media}, flags {flags}")


def test_texel_corners_when_roughness_is_the_only_texture(api, oracle_mod):
    """the colour textures stripped: the scene is still a textured scene (UVs, tables, TEX variants, queued shadow rays)"""
    c = _room(oracle_mod, "stripped", lambda: RC.corner_room(W, H, keep_colour=False))
    assert all(m.material.texture is None for m in c["tex"].models)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    _check_render(r, c, "roughness only")


def test_texel_corners_under_flat_normal_maps(api, oracle_mod):
    """a flat normal map on every surface: the normal-map variants of the surface passes, whose normal is the plain one bit for bit"""
    from normalmap_common import flat_texture
    c = _corner(oracle_mod)
    mapped, _ = RC.corner_room(W, H, normal=flat_texture(2, 2))
    r = api.Renderer(mapped, W, H, max_bounces=DEPTH)
    _check_render(r, c, "flat normal maps")


def test_texel_corners_under_a_lens(api, oracle_mod):
    from test_gpu_lens import Expect
    mapped, plain = RC.corner_room(W, H, lens=True)
    ex = Expect(oracle_mod, "roughness corner", lens=LENS, w=W, h=H, depth=DEPTH, scene=plain)
    r = api.Renderer(mapped, W, H, max_bounces=DEPTH)
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
    o, d, key, sample = _random_rays(np.array([-10, -10, -10, 10, 10, 10], F), 1000, 17)
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
    m = luminance(acc) / F(2.0)
    rel = np.sqrt(np.maximum(q / F(2.0) - m * m, 0) / F(2.0)) / np.maximum(m, F(1e-3))
    crit = dict(rel_error=float(np.quantile(rel[rel > 0], 0.5)), abs_floor=0.0, min_samples=2, max_samples=0)
    assert r.render_adaptive(2, **crit) == W * H
    assert_bit_equal(r.read_frame()[0], acc, "adaptive round 1"); assert_bit_equal(r.read_moments(), q, "adaptive moments")
    want = criterion(acc, q, **crit)
    assert 0 < want.sum() < W * H, "the criterion should split the frame"
    assert r.render_adaptive(2, **crit) == int(want.sum())
    acc4 = (acc + s[2]) + s[3]
    assert_bit_equal(r.read_frame()[0], np.where(want[..., None], acc4, acc), "adaptive round 2")


def test_texel_corners_after_a_move_on_the_patch_path(api, oracle_mod):
    from instances_common import apply, move, shifted
    c = _corner(oracle_mod)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    r.render(0, 1)
    before = r.scene_info()
    slab = next(i for i, m in enumerate(c["tex"].models) if m.name == "slab")                 # a roughness-mapped model moves
    step = [(slab, shifted(c["tex"].models[slab].matrices, (-1.0, 0.5, 1.0)))]
    move(r, step)
    got = r.render_samples(0, SPP)
    after = r.scene_info()
    assert (after.uploads_patched, after.uploads_full, after.blas_builds) == (before.uploads_patched + 1, before.uploads_full, before.blas_builds)
    want = oracle_mod.Oracle(apply(c["plain"], step)).render_samples(W, H, SPP, max_bounces=DEPTH)
    assert_bit_equal(got, want, "moved roughness-mapped scene")


def test_the_setter_on_a_live_renderer_and_clearing(api, oracle_mod):
    """a renderer of the colour-textured room that has rendered: the map set by the setter gives the mapped frame (one full upload, no BLAS or
    TLAS build), clearing it gives back the frame of the room that never had one"""
    from textures_common import corner_scene
    c = _corner(oracle_mod)
    tex, plain = corner_scene(W, H)
    never = oracle_mod.Oracle(plain).render_samples(W, H, SPP, max_bounces=DEPTH)
    r = api.Renderer(tex, W, H, max_bounces=DEPTH)
    assert_bit_equal(r.render_samples(0, SPP), never, "before the setter")
    i0 = r.scene_info()
    t = r.add_texture(RC.corner_map().data)
    mats = sorted({r._materials.index(m.material) for m in tex.models if m.material.kind in RC.GGX_KINDS})
    assert len(mats) == 2
    for mi in mats:
        r.set_material_roughness_texture(mi, t)
    r.rebuild()
    assert_bit_equal(r.render_samples(0, SPP), c["samples"][:SPP], "after the setter")
    i1 = r.scene_info()
    assert (i1.blas_builds, i1.tlas_builds, i1.uploads_full) == (i0.blas_builds, i0.tlas_builds, i0.uploads_full + 1)
    assert not np.array_equal(c["samples"][:SPP], never), "the map changes the picture"
    for mi in mats:
        r.set_material_roughness_texture(mi, -1)
    r.rebuild()
    assert_bit_equal(r.render_samples(0, SPP), never, "after clearing")


# ---- 2. a constant map at varying UVs is the material of that roughness
def test_a_constant_map_at_random_uvs_renders_as_that_roughness(api, oracle_mod):
    c = _room(oracle_mod, "constant", lambda: RC.random_uv_room(W, H))
    assert any(m.material.roughness_texture is not None and abs(m.material.roughness - 0.45) > 0.05 for m in c["tex"].models)
    r = api.Renderer(c["tex"], W, H, max_bounces=DEPTH)
    _check_render(r, c, "constant map")


# ---- 3. a map that varies across a triangle: every quad hit shaded by an oracle whose material has the hit's roughness
def varying_quad(kind, rmap=None):
    """normalmap_common.quad_scene's geometry, UVs, camera and light; the quad GGX metal (or a GGX dielectric without a volume) of roughness
    0.35 under a 5 x 3 map of distinct r values in [0.1, 0.9]"""
    from normalmap_common import quad_scene
    from path_tracer_amd.scene_desc import GGX, SceneDesc
    material = GGX.new_metal((0.9, 0.75, 0.6), 0.35) if kind == "metal" else GGX.new_dielectric((0.9, 0.75, 0.6), 0.35, 1.5)
    base = quad_scene(QW, QH, material)
    quad = dataclasses.replace(base.models[0], material=material.roughness_mapped(RC.varied_map(5, 3, 9) if rmap is None else rmap))
    return SceneDesc.new([quad] + list(base.models[1:]), base.camera, "roughness-mapped quad")


def quad_hits(orc, desc):
    """the camera samples of varying_quad's description that hit the quad first, from the oracle's side alone: (sample, pixel, o, d, hit) and
    the restated linear roughness rho of each"""
    inst_model = world_instance_models(desc)
    out = dict(s=[], p=[], o=[], d=[], hit=[], rho=[])
    for s in range(QSPP):
        for p in range(QW * QH):
            o, d = orc.primary_ray(QW, QH, p, s)
            hit = orc.trace_closest(o[None], d[None])
            if hit["inst"][0] == 0xFFFFFFFF or inst_model[hit["inst"][0]] != 0:
                continue
            out["s"].append(s); out["p"].append(p); out["o"].append(o); out["d"].append(d); out["hit"].append(hit)
            out["rho"].append(RC.scene_rho(desc, hit["inst"], hit["prim"], hit["u"], hit["v"])[0])
    out["rho"] = np.array(out["rho"], F)
    return out


def composed(oracle_mod, desc, nee):
    """every sample at max_bounces = 1: a hit on the quad is normalmap_common.composed_sample with the oracle's own normal, on an Oracle whose
    material 0 has roughness = the hit's restated rho (one per distinct rho); everything else is the oracle's integrate()"""
    from normalmap_common import composed_sample
    from path_tracer_amd.scene_desc import Material, SceneDesc
    plain = RC.untextured(desc)
    orc = oracle_mod.Oracle(plain)
    hits = quad_hits(orc, desc)
    want = np.zeros((QSPP, QH, QW, 4), F)
    for s in range(QSPP):
        for p in range(QW * QH):
            o, d = orc.primary_ray(QW, QH, p, s)
            want[s, p // QW, p % QW] = orc.integrate(o, d, p, s, 1, max_bounces=1, enable_nee=int(nee))[0]
    by_rho = {}
    mat = plain.models[0].material
    for k in range(len(hits["s"])):
        rho = hits["rho"][k]
        bits = int(rho.view(np.uint32))
        if bits not in by_rho:
            m0 = dataclasses.replace(plain.models[0], material=Material(mat.kind, mat.colour, float(rho), mat.ior, mat.volume))
            by_rho[bits] = oracle_mod.Oracle(SceneDesc.new([m0] + list(plain.models[1:]), plain.camera))
        s, p, hit = hits["s"][k], hits["p"][k], hits["hit"][k]
        want[s, p // QW, p % QW] = composed_sample(by_rho[bits], plain, plain.models[1], hits["o"][k], hits["d"][k], p, s, hit, hit["normal"][0],
                                                   int(hit["front"][0]), nee)
    return want, hits, orc


@pytest.mark.parametrize("nee", [False, True], ids=["no_nee", "nee"])
@pytest.mark.parametrize("kind", ["metal", "dielectric"])
def test_a_varying_map_composes_from_oracle_pieces(api, oracle_mod, kind, nee):
    desc = varying_quad(kind)
    want, hits, orc = composed(oracle_mod, desc, nee)
    assert len(hits["rho"]) > QW * QH * QSPP // 3
    texels = desc.models[0].material.roughness_texture.data[..., 0].reshape(-1)
    assert (hits["rho"] != F(0.35)).all() and not np.isin(hits["rho"], texels).any()
    # the map matters: the unmapped quad (roughness 0.35 everywhere) is another picture
    unmapped = orc.render_samples(QW, QH, QSPP, max_bounces=1, enable_nee=int(nee))
    assert (unmapped != want).any()
    r = api.Renderer(desc, QW, QH, max_bounces=1, enable_nee=nee)
    assert_bit_equal(r.render_samples(0, QSPP), want, f"{kind}, nee {nee}: composed samples")


# ---- 4. the unit hook on the device
def test_surface_roughness_on_the_device_is_the_host_evaluation(api):
    desc = RC.hook_scene()
    r = api.Renderer(desc, 16, 16)
    q = RC.hook_queries(desc)
    host = r.surface_roughness(*q)
    assert_bit_equal(host, RC.scene_alpha(desc, *q), "the host evaluation is the definition")
    assert_bit_equal(r.surface_roughness(*q, on_device=True), host, "surface roughness, device")
    plain = api.Renderer(RC.untextured(desc), 16, 16)                                       # no texture view at all on the device
    got = plain.surface_roughness(*q, on_device=True)
    assert_bit_equal(got, plain.surface_roughness(*q), "untextured scene")
    assert (got != host).any() and (got > 0).any()


# ---- 5. the baked view: the metal ending reads the alpha at the hit
BW, BH, BDEPTH = 37, 19, 3
UNLIT = (0.25, 0.5, 0.125)
ALPHAS5 = (0.1, 0.2, 0.4, 0.7, 1.0)
_BAKED = {}


def _baked_room(O):
    """the mapped room of tests/test_gpu_probe_radiance.py (its panel GGX metal beside the unmapped metal floor) with a 4 x 4 roughness map of
    distinct values on both metals: the panel's UVs vary, the floor has none and reads texel (0, 0)"""
    if not _BAKED:
        import baked_common as BC
        import probe_depth_common as PD
        import probe_grid_common as PG
        import probe_radiance_common as PR
        from path_tracer_amd.scene_desc import GGX
        sc, maps = BC.mapped_room(BW, BH)
        sc.models[BC.MAPPED_MODELS.index("panel")].material = GGX.new_metal((0.6, 0.9, 0.5), 0.6)
        sc = RC.with_roughness(sc, RC.varied_map(4, 4, 5, lo=0.2, hi=0.95), kinds=(3,))
        grid = PG.room_grid()
        _BAKED.update(scene=sc, maps=maps, grid=grid, depth=PD.random_depth(grid, 4, 61, 0.0, True), rad=PR.random_radiance(grid, 8, ALPHAS5, 63),
                      oracle=O.Oracle(sc))
    return _BAKED


@pytest.mark.parametrize("depth", [False, True], ids=["plain", "vis"])
def test_the_baked_views_metal_ending_reads_the_alpha_at_the_hit(api, oracle_mod, depth):
    import baked_common as BC
    import guides_follow_common as G
    import probe_radiance_common as PR
    room = _baked_room(oracle_mod)
    follow, sample = 2, 0
    o, d = G.pinhole_rays(room["oracle"], BW, BH, sample)
    dv = room["depth"] if depth else None
    want, ending, on_metal, alpha = RC.baked(room["oracle"], room["scene"], room["maps"], room["grid"], dv, room["rad"], o, d, follow, UNLIT)
    flat, _, _, flat_alpha = RC.baked(room["oracle"], room["scene"], room["maps"], room["grid"], dv, room["rad"], o, d, follow, UNLIT, mapped=False)
    # the unmapped restatement is probe_radiance_common's own
    theirs, _, _ = PR.baked(room["oracle"], RC.untextured_roughness(room["scene"]), room["maps"], room["grid"], dv, room["rad"], o, d, follow, UNLIT)
    assert_bit_equal(flat, theirs, "the restatement without maps is the existing one")
    shiny = np.isin(ending, (PR.METAL_FRONT, PR.METAL_BACK))
    assert shiny.sum() > 0.05 * BW * BH, "the metal is the final surface of more than 5 % of the pixels"
    levels = set(PR.level_of(room["rad"], alpha[shiny])[0].tolist())
    assert len(levels) >= 2, "the restated alphas span at least two prefilter levels"
    assert (alpha[shiny] != flat_alpha[shiny]).any() and (want != flat).any(axis=1).any(), "the map changes the picture"
    assert np.array_equal(want[~shiny].view(np.uint32), flat[~shiny].view(np.uint32)), "... and only on the metal"
    r = api.Renderer(room["scene"], BW, BH, max_bounces=BDEPTH)
    BC.set_maps(r, room["maps"])
    room["grid"].set_on(r)
    if depth:
        room["depth"].set_on(r)
    room["rad"].set_on(r)
    r.reset_baked()
    s = r.render_baked(sample, 1, follow=follow, unlit=UNLIT)
    assert (s[..., 3] == 1).all()
    assert_bit_equal(s[..., :3], want.reshape(BH, BW, 3), f"baked view, depth {depth}")


# ---- 6. the C++ driver
def test_headless_roughness_checker_writes_what_the_python_route_presents(api, tmp_path):
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import GGX, Model, SceneDesc, Texture
    from test_gpu_post import _read_png
    n, w, h = 4, 32, 32
    exe = B.build_host_driver()
    out = tmp_path / "roughness.png"
    run = subprocess.run([exe, "--width", str(w), "--height", str(h), "--bounces", str(DEPTH), "--render", "0", "3", "--metal-box", "--roughness-checker", str(n),
                          "--out", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    tex = Texture.new(np.repeat(np.where((i + j) & 1, F(0.6), F(0.1))[..., None], 3, axis=2))
    metal = GGX.new_metal((0.9, 0.8, 0.6), 0.4)
    src = scenes.cornell_models(tall_material=metal)
    assert [m.name for m in src][4] == "cb_box_tall"
    paths = [os.path.join(ROOT, "models", "cornell", m.name + ".obj") for m in src]
    models = [Model.from_obj(p, m.material.roughness_mapped(tex) if m.name == "cb_box_tall" else m.material) for p, m in zip(paths, src)]
    r = api.Renderer(SceneDesc.new(models, scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    p, _ = r.model_vertices(4)
    xz = p[:, :, [0, 2]]
    lo, hi = xz.min(axis=(0, 1)), xz.max(axis=(0, 1))
    r.set_model_uvs(4, (xz - lo) / (hi - lo))
    r.rebuild()
    r.render(0, 3)
    assert np.array_equal(_read_png(out), r.present_rgb8().reshape(h, w, 3))
    plain = api.Renderer(SceneDesc.new([Model.from_obj(p, m.material) for p, m in zip(paths, src)], scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    plain.render(0, 3)
    assert not np.array_equal(plain.present_rgb8(), r.present_rgb8())
    # the flag is refused without the box it maps
    bad = subprocess.run([exe, "--roughness-checker", "4"], capture_output=True, text=True, cwd=ROOT, timeout=60)
    assert bad.returncode == 2 and "--metal-box" in bad.stderr
