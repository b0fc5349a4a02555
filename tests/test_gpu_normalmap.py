"""GPU: normal maps (pt_set_material_normal_texture), checked the ways the oracle allows, since it knows nothing of textures: a FLAT map is the
plain scene, bit for bit, through every route; a varying map composes from oracle pieces with the numpy restatement of N' in them; the unit hook
on the device is its host evaluation; a constant tilt is (all but last-bit rounding) the scene with tilted vertex normals; the C++ driver writes
what the Python route presents.  tests/normalmap_common.py holds the restatement and the scenes."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from instances_common import apply, move, shifted
from normalmap_common import F, composed_samples, flat_texture, hook_queries, hook_scene, quad_scene, tilt_normal, tilt_scene
from textures_common import corner_scene, world_instance_models

pytestmark = pytest.mark.gpu

W, H, DEPTH, SPP = 16, 12, 6, 2
LENS = (0.6, 9.0)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def flat_mapped(desc):
    """desc with ONE flat 4 x 2 normal map on every material that can carry one; a model without UVs gets UVs that vary across its triangles
    (a flat map is the plain normal wherever it is looked up)"""
    from path_tracer_amd.scene_desc import SceneDesc
    flat = flat_texture(4, 2)
    rng = np.random.default_rng(21)
    mapped = {}
    models = []
    for m in desc.models:
        if m.material.kind == 1:
            models.append(m)
            continue
        if m.material not in mapped:
            mapped[m.material] = m.material.normal_mapped(flat)
        uvs = m.uvs if m.uvs is not None else rng.uniform(-2.0, 3.0, (m.positions.shape[0], 3, 2)).astype(F)
        models.append(dataclasses.replace(m, material=mapped[m.material], uvs=uvs))
    return SceneDesc.new(models, desc.camera, desc.name + ", flat normal maps")


_CACHE = {}


def _corner(oracle_mod, glass=True):
    """§13's closed room of ten models: the untextured description under flat maps, the texel-corner one under flat maps, and the oracle's
    render of the untextured one, computed once"""
    key = "corner" if glass else "corner, no media"
    if key not in _CACHE:
        tex, plain = corner_scene(W, H, media=glass)
        orc = oracle_mod.Oracle(plain)
        samples = orc.render_samples(W, H, SPP + 2, max_bounces=DEPTH)
        frame = orc.render(W, H, SPP, max_bounces=DEPTH)
        _CACHE[key] = dict(flat=flat_mapped(plain), both=flat_mapped(tex), plain=plain, orc=orc, samples=samples, frame=frame)
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


# ---- 4. a flat map is the plain scene, through every route
@pytest.mark.parametrize("flags", [0, 2, 16], ids=["lds", "no_lds_scene", "general_walk"])
def test_flat_maps_render_as_the_plain_scene(api, oracle_mod, flags):
    c = _corner(oracle_mod)
    r = api.Renderer(c["flat"], W, H, max_bounces=DEPTH, flags=flags)
    _check_render(r, c, f"flags {flags}")
    assert r.stats().lds_scene == (0 if flags == 2 else 1)


@pytest.mark.parametrize("flags", [0, 2], ids=["lds", "no_lds_scene"])
def test_flat_maps_on_top_of_colour_textures_at_texel_corners(api, oracle_mod, flags):
    c = _corner(oracle_mod)
    r = api.Renderer(c["both"], W, H, max_bounces=DEPTH, flags=flags)
    _check_render(r, c, f"colour textures too, flags {flags}")


def test_flat_maps_without_media(api, oracle_mod):
    """the same room without the glass boxes: the normal-map variants WITHOUT media (the room with the glass runs only those with)"""
    c = _corner(oracle_mod, glass=False)
    r = api.Renderer(c["flat"], W, H, max_bounces=DEPTH)
    _check_render(r, c, "no media")
    rb = api.Renderer(c["both"], W, H, max_bounces=DEPTH)
    _check_render(rb, c, "no media, colour textures too")


@pytest.mark.parametrize("glass", [True, False], ids=["media", "no_media"])
def test_flat_maps_share_a_scene_with_textured_lights(api, oracle_mod, glass):
    """section 18's room of lamps at texel corners under flat maps: the normal-map variants WITH an emission texture, against the oracle's
    render of the equivalent untextured scene"""
    from emission_common import emission_corner_scene
    tex, plain = emission_corner_scene(W, H, media=glass)
    orc = oracle_mod.Oracle(plain)
    c = dict(samples=orc.render_samples(W, H, SPP, max_bounces=DEPTH), frame=orc.render(W, H, SPP, max_bounces=DEPTH))
    r = api.Renderer(flat_mapped(tex), W, H, max_bounces=DEPTH)
    _check_render(r, c, f"textured lights, media {glass}")


def test_flat_maps_under_a_lens(api, oracle_mod):
    from test_gpu_lens import Expect
    _, plain = corner_scene(W, H, lens=True)
    ex = Expect(oracle_mod, "corner", lens=LENS, w=W, h=H, depth=DEPTH, scene=plain)
    r = api.Renderer(flat_mapped(plain), W, H, max_bounces=DEPTH)
    assert_bit_equal(r.render_samples(0, SPP), ex.samples(0, SPP), "lens: per-sample radiance")
    r.reset_accumulation()
    got = r.render(0, SPP)
    want = ex.frame(SPP)
    assert_bit_equal(got[0], want[0], "lens: accumulation"); assert_bit_equal(got[1], want[1], "lens: position")
    assert np.array_equal(got[2], want[2])


def test_flat_maps_through_caller_rays(api, oracle_mod):
    from test_gpu_rays import _oracle_rays, _random_rays
    c = _corner(oracle_mod)
    r = api.Renderer(c["flat"], W, H, max_bounces=DEPTH)
    o, d, key, sample = _random_rays(np.array([-10, -10, -10, 10, 10, 10], F), 600, 17)
    got = r.integrate_rays(o, d, key, sample, draws_consumed=1)
    want = _oracle_rays(c["orc"], o, d, key, sample, 1, DEPTH)
    assert_bit_equal(got[0], want[0], "rays: radiance"); assert_bit_equal(got[1], want[1], "rays: position")
    assert np.array_equal(got[2], want[2])


def test_flat_maps_adaptive_round(api, oracle_mod):
    from test_adaptive_host import criterion, luminance
    c = _corner(oracle_mod)
    s = c["samples"]
    r = api.Renderer(c["flat"], W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
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


def test_flat_maps_on_two_contexts(api, oracle_mod):
    c = _corner(oracle_mod)
    m = api.MultiRenderer(c["flat"], W, H, [0, 0], max_bounces=DEPTH, strip_rows=4)
    got = m.render(0, SPP)
    m.close()
    assert_bit_equal(got, c["frame"][0], "pt_multi over a duplicated device")


def test_flat_maps_after_a_patched_move_and_the_setters_upload(api, oracle_mod):
    c = _corner(oracle_mod)
    r = api.Renderer(c["flat"], W, H, max_bounces=DEPTH)
    r.render(0, 1)
    before = r.scene_info()
    tall = next(i for i, m in enumerate(c["flat"].models) if m.name == "tall")
    step = [(tall, shifted(c["flat"].models[tall].matrices, (-2.0, 0.5, 1.0)))]
    move(r, step)
    got = r.render_samples(0, SPP)
    after = r.scene_info()
    assert (after.uploads_patched, after.uploads_full, after.blas_builds) == (before.uploads_patched + 1, before.uploads_full, before.blas_builds)
    want = oracle_mod.Oracle(apply(c["plain"], step)).render_samples(W, H, SPP, max_bounces=DEPTH)
    assert_bit_equal(got, want, "moved scene under flat maps")
    # the setter: no BLAS, no TLAS, and the next upload is a full one; a move after THAT is patched again
    mats = sorted({r._materials.index(m.material) for m in c["flat"].models if m.material.normal_texture is not None})
    r.set_material_normal_texture(mats[0], -1); r.rebuild()
    assert_bit_equal(r.render_samples(0, 1), want[:1], "one map cleared")
    cleared = r.scene_info()
    assert (cleared.uploads_patched, cleared.uploads_full, cleared.blas_builds, cleared.tlas_builds) == (
        after.uploads_patched, after.uploads_full + 1, after.blas_builds, after.tlas_builds)
    move(r, [(tall, c["flat"].models[tall].matrices)])
    assert_bit_equal(r.render_samples(0, SPP), c["samples"][:SPP], "moved back")
    back = r.scene_info()
    assert (back.uploads_patched, back.uploads_full, back.blas_builds) == (cleared.uploads_patched + 1, cleared.uploads_full, cleared.blas_builds)


# ---- 5. a varying map: the sample composed from oracle pieces
CW = CH = 8


def _compose(api, oracle_mod, material, nee):
    """render_samples of quad_scene at max_bounces = 1 beside the composition from oracle pieces (normalmap_common.composed_samples)"""
    desc = quad_scene(CW, CH, material)
    r = api.Renderer(desc, CW, CH, max_bounces=1, enable_nee=nee)
    t = r.tlas_instances(0)
    got = r.render_samples(0, SPP)
    want, n_quad, n_moved = composed_samples(oracle_mod, desc, t["matrix"], t["inv_matrix"], CW, CH, SPP, nee)
    assert n_quad > CW * CH * SPP // 3 and n_moved == n_quad, "the map perturbs every hit on the quad"
    return got, want


@pytest.mark.parametrize("nee", [False, True], ids=["no_nee", "nee"])
@pytest.mark.parametrize("kind", ["lambertian", "specular", "ggx_metal"])
def test_a_varying_map_composes_from_oracle_pieces(api, oracle_mod, kind, nee):
    """NEE off: one bounce off the quad at the restated N'.  NEE on, under the small light: also both direct-light estimates, the explicit one
    with pt_bsdf_eval at the sampled light direction and N', the BSDF-sampled one with pt_material_eval at N' (a mirror has neither)"""
    from path_tracer_amd.scene_desc import GGX, Lambertian, Specular
    material = dict(lambertian=Lambertian.new((0.9, 0.8, 0.7)), specular=Specular.new((0.9, 0.85, 0.8)),
                    ggx_metal=GGX.new_metal((0.9, 0.75, 0.6), 0.35))[kind]
    got, want = _compose(api, oracle_mod, material, nee)
    assert_bit_equal(got, want, f"{kind}, nee {nee}: composed samples")


# ---- 6. the unit hook on the device
@pytest.mark.parametrize("flat", [False, True], ids=["bumpy", "flat"])
def test_shading_normal_on_the_device_is_the_host_evaluation(api, flat):
    desc = hook_scene(flat=flat)
    r = api.Renderer(desc, 16, 16)
    q = hook_queries(desc)
    host, hfront = r.shading_normal(*q)
    dev, dfront = r.shading_normal(*q, on_device=True)
    assert_bit_equal(dev, host, "shading normal, device"); assert np.array_equal(dfront, hfront)
    never = type(desc).new([dataclasses.replace(m, material=m.material.normal_mapped(None).textured(None)) if m.material.kind != 1 else m
                            for m in desc.models], None, "no texture view at all on the device")
    rn = api.Renderer(never, 16, 16)
    pd, pf = rn.shading_normal(*q, on_device=True)
    ph, phf = rn.shading_normal(*q)
    assert_bit_equal(pd, ph, "unmapped scene"); assert np.array_equal(pf, phf)
    if flat:
        assert_bit_equal(dev, pd, "flat maps are the plain normal on the device too")


# ---- 7. a constant tilt is the tilted-normal scene
# relative difference of the image mean between two oracle renders (seeds 1 and 2) of the tilted-vertex-normal floor at 16 x 16, 64 spp: the
# noise of the mean itself.  Three times that is allowed between the mapped render and the oracle's vertex-normal one (same seed: they differ
# by the last-bit rounding of unit3 over equal vertex normals, so this is a sanity bound on a mean, not a parity claim)
SEED_SPREAD = 0.0012449434441821434  # measured (the oracle, seeds 1 and 2; profiles/r18_normal_maps.md); the test measures it again and compares


def _mean(img):
    return float(img[..., :3].astype(np.float64).mean())


def test_a_constant_tilt_is_the_tilted_vertex_normal_scene(api, oracle_mod):
    w = h = 16
    spp = 64
    n = tilt_normal()
    up = np.array([0.0, 1.0, 0.0], F)
    assert not np.array_equal(n, up) and abs(float(np.sqrt((n.astype(np.float64) ** 2).sum())) - 1.0) < 1e-6
    vertex = tilt_scene(w, h, n)
    orc = oracle_mod.Oracle(vertex)
    ref = _mean(orc.render(w, h, spp, max_bounces=DEPTH)[0])
    a = _mean(orc.render(w, h, spp, max_bounces=DEPTH, seed=1)[0])
    b = _mean(orc.render(w, h, spp, max_bounces=DEPTH, seed=2)[0])
    spread = abs(a - b) / (0.5 * (a + b))
    print(f"seed spread of the image mean: {spread:.6f} (recorded: {SEED_SPREAD})")
    assert abs(spread - SEED_SPREAD) <= 1e-6 * SEED_SPREAD, "the oracle is deterministic: the recorded measurement is this one"
    tol = 3.0 * SEED_SPREAD
    r = api.Renderer(tilt_scene(w, h, "map"), w, h, max_bounces=DEPTH)
    mapped = _mean(r.render(0, spp)[0])
    rf = api.Renderer(tilt_scene(w, h, "flat"), w, h, max_bounces=DEPTH)
    flat = _mean(rf.render(0, spp)[0])
    print(f"image means: mapped {mapped:.6f}, oracle vertex normals {ref:.6f} (rel {abs(mapped - ref) / ref:.2e}), flat {flat:.6f} (rel {abs(flat - mapped) / mapped:.2e}); tol {tol:.2e}")
    assert abs(mapped - ref) / ref <= tol
    assert abs(flat - mapped) / mapped > tol, "a map that is ignored must not pass"


# ---- 8. the C++ driver
def ripple_texture(n):
    """examples/headless --normal-ripples N, one binary32 operation per step as the driver writes it"""
    from path_tracer_amd.scene_desc import Texture
    i = np.arange(n, dtype=F)
    a = (i + F(0.5)) / F(n)
    tri = F(0.3) * (F(4.0) * np.abs(a - F(0.5)) - F(1.0))
    x, y = np.meshgrid(tri, tri)                                       # texel (i, j): x from the column i, y from the row j
    z = np.sqrt((F(1.0) - x * x) - y * y)
    return Texture.new(F(0.5) * np.stack([x, y, z], axis=2).astype(F) + F(0.5))


def test_headless_normal_ripples_writes_what_the_python_route_presents(api, tmp_path):
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    from test_gpu_post import _read_png
    n, w, h = 8, 16, 16
    exe = B.build_host_driver()
    out = tmp_path / "ripples.png"
    run = subprocess.run([exe, "--width", str(w), "--height", str(h), "--bounces", str(DEPTH), "--render", "0", "3", "--normal-ripples", str(n), "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr
    tex = ripple_texture(n)
    src = scenes.cornell_models()
    assert [m.name for m in src][1] == "cb_main"
    models = [Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material.normal_mapped(tex) if m.name == "cb_main" else m.material)
              for m in src]
    r = api.Renderer(SceneDesc.new(models, scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    p, _ = r.model_vertices(1)
    st = np.stack([p[:, :, 0], p[:, :, 1] + p[:, :, 2]], axis=2)
    lo, hi = st.min(axis=(0, 1)), st.max(axis=(0, 1))
    r.set_model_uvs(1, (st - lo) / (hi - lo))
    r.rebuild()
    r.render(0, 3)
    assert np.array_equal(_read_png(out), r.present_rgb8().reshape(h, w, 3))
    plain = api.Renderer(SceneDesc.new([Model.from_obj(m.obj_path, s.material) for m, s in zip(models, src)], scenes.reference_camera(w / h)), w, h, max_bounces=DEPTH)
    plain.render(0, 3)
    assert not np.array_equal(plain.present_rgb8(), r.present_rgb8())
