"""GPU (-m gpu): lightmaps kept by the context and the baked view (pt_lightmap_lookup on the device, pt_render_baked), bit for bit unless
said.  The expected values are the definition restated over oracle pieces (baked_common.baked: primary_ray, trace_closest per hop, the
restated surface colour, the follow-on direction, the numpy lookup); the guides and pt_render_samples where the view must equal them; and
one statistical test that a baked view means what the bake means: the picture of a baked room against the path-traced one."""
import ctypes as C

import numpy as np
import pytest

import baked_common as BC
import guides_follow_common as G
import lightmap_common as LC
from conftest import assert_bit_equal
from path_tracer_amd.scene_desc import EMISSIVE, Camera

pytestmark = pytest.mark.gpu
F = np.float32
MISS = 0xFFFFFFFF
W, H = 37, 19             # several waves with a ragged last block
DEPTH = 3
UNLIT = (0.25, 0.5, 0.125)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_ROOM = {}


def _room(O=None):
    """the mapped room at W x H, its maps, its oracle and the oracle's camera rays per sample: made once and left unchanged"""
    if "scene" not in _ROOM:
        _ROOM["scene"], _ROOM["maps"] = BC.mapped_room(W, H)
        _ROOM["rays"], _ROOM["want"] = {}, {}
    if O is not None and "oracle" not in _ROOM:
        _ROOM["oracle"] = O.Oracle(_ROOM["scene"])
    return _ROOM


def _want(O, sample, hops, unlit=UNLIT):
    room = _room(O)
    key = (sample, hops, tuple(unlit))
    if key not in room["want"]:
        if sample not in room["rays"]:
            room["rays"][sample] = G.pinhole_rays(room["oracle"], W, H, sample)
        B, ending = BC.baked(room["oracle"], room["scene"], room["maps"], *room["rays"][sample], hops, unlit)
        room["want"][key] = B.reshape(H, W, 3), ending.reshape(H, W)
    return room["want"][key]


def _one(r, sample, follow, unlit=(0.0, 0.0, 0.0)):
    """the baked sample of `sample` alone: fresh sums, so S.rgb = 0 + B = B and S.w = 1"""
    r.reset_baked()
    s = r.render_baked(sample, 1, follow=follow, unlit=unlit)
    assert (s[..., 3] == 1).all()
    return s[..., :3]


# ---- 1. the lookup on the device
def test_device_lookup_is_the_host_lookup(api):
    sc, maps = BC.soup_scene()
    r = api.Renderer(sc, 48, 32)
    BC.set_maps(r, maps)
    q = BC.soup_queries(sc)                      # 777 queries: more than one block, not a multiple of it
    host, dev = r.lightmap_lookup(*q), r.lightmap_lookup(*q, on_device=True)
    assert_bit_equal(dev[0], host[0], "soup")
    assert np.array_equal(dev[1], host[1]) and host[1].any() and not host[1].all()
    # the tables follow the maps: clearing one and setting another shows at once
    r.set_lightmap(1, 0, None)
    r.set_lightmap(1, 2, maps[1, 0])
    host, dev = r.lightmap_lookup(*q), r.lightmap_lookup(*q, on_device=True)
    assert_bit_equal(dev[0], host[0], "soup, maps changed")
    assert np.array_equal(dev[1], host[1]) and not host[1][q[0] == 1].any() and host[1][q[0] == 3].all()
    sc = BC.clamp_scene()
    r = api.Renderer(sc, 48, 32)
    r.set_lightmap(0, 0, np.random.default_rng(3).uniform(0.0, 1.0, (3, 5, 3)).astype(F))
    k = len(BC.CLAMP_UVS)
    q = (np.zeros(k, np.uint32), np.arange(k, dtype=np.uint32), np.full(k, 0.3, F), np.full(k, 0.2, F))
    assert_bit_equal(r.lightmap_lookup(*q, on_device=True)[0], r.lightmap_lookup(*q)[0], "clamp")
    sc = BC.centre_scene(16, 16)
    r = api.Renderer(sc, 48, 32)
    tex = np.random.default_rng(4).uniform(0.0, 1.0, (16, 16, 3)).astype(F)
    r.set_lightmap(0, 0, tex)
    q = (np.zeros(256, np.uint32), np.arange(256, dtype=np.uint32), np.full(256, 0.125, F), np.full(256, 0.5, F))
    assert_bit_equal(r.lightmap_lookup(*q, on_device=True)[0].reshape(16, 16, 3), tex, "texel centres on the device")


def test_device_lookup_with_one_unmapped_triangle_in_front(api, oracle_mod):
    """the compact UV table of an untextured scene starts one triangle below the mapped models' triangles here: the word that leads a leaf to
    its UVs is then all ones, and says nothing about whether the leaf is mapped; two placements of one model share one copy of its UVs"""
    sc, maps = BC.offset_scene()
    r = api.Renderer(sc, 48, 32)
    BC.set_maps(r, maps)
    q = BC.offset_queries(sc)
    want, want_mapped = BC.scene_lookup(sc, maps, *q)
    host, dev = r.lightmap_lookup(*q), r.lightmap_lookup(*q, on_device=True)
    assert np.array_equal(want_mapped, (q[0] > 0).astype(np.uint8)) and all((q[0] == k).sum() > 30 for k in range(4))
    assert np.array_equal(host[1], want_mapped) and np.array_equal(dev[1], want_mapped)
    assert_bit_equal(host[0], want, "host")
    assert_bit_equal(dev[0], want, "device")
    # ... and the view: the kernel reads the same records
    orc = oracle_mod.Oracle(sc)
    B, ending = BC.baked(orc, sc, maps, *G.pinhole_rays(orc, 48, 32, 0), 0, UNLIT)
    assert (ending == BC.MAPPED_FRONT).sum() > 30 and (ending == BC.MAPPED_BACK).sum() > 30
    assert_bit_equal(_one(r, 0, 0, UNLIT), B.reshape(32, 48, 3), "the view")


def test_device_round_trip_with_the_bakes_convention(api):
    """tests/test_baked_host.py's round trip on the device: a multi-model scene, the mapped model's triangles well inside the flattened scene"""
    sc, model = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)
    tex = np.random.default_rng(6).uniform(0.0, 1.0, (16, 16, 3)).astype(F)
    r.set_lightmap(model, 0, tex)
    prim, uv, _, _ = r.lightmap_texels(model, 0, 16, 16)
    cov = prim != LC.MISS
    leaf = [k for k, (m, _) in enumerate(BC.leaf_keys(sc)) if m == model][0]
    q = (np.full(cov.sum(), leaf, np.uint32), prim[cov], uv[cov][:, 0], uv[cov][:, 1])
    dev, host = r.lightmap_lookup(*q, on_device=True), r.lightmap_lookup(*q)
    assert_bit_equal(dev[0], host[0], "round trip on the device")
    assert dev[1].all() and np.abs(dev[0].astype(np.float64) - tex[cov]).max() < 1e-3


def test_device_lookup_in_a_textured_scene_uses_its_uv_table(api):
    """a textured scene holds every model's UVs in the texture tables already: the lightmap tables reuse them"""
    from textures_common import varying_scene
    sc = varying_scene(48, 32)
    r = api.Renderer(sc, 48, 32)
    floor = [m.name for m in sc.models].index("floor")
    tex = np.random.default_rng(8).uniform(0.0, 1.0, (3, 5, 3)).astype(F)
    r.set_lightmap(floor, 0, tex)
    n = 300
    rng = np.random.default_rng(9)
    inst = rng.integers(0, len(sc.models), n).astype(np.uint32)
    prim = rng.integers(0, 2, n).astype(np.uint32)
    u = rng.uniform(0, 1, n).astype(F); v = (rng.uniform(0, 1, n) * (1 - u)).astype(F)
    want, want_mapped = BC.scene_lookup(sc, {(floor, 0): tex}, inst, prim, u, v)
    got, mapped = r.lightmap_lookup(inst, prim, u, v, on_device=True)
    assert_bit_equal(got, want, "textured scene")
    assert np.array_equal(mapped, want_mapped) and mapped.any()


# ---- 2. without maps and with unlit = 1 the view is the albedo guide
@pytest.mark.parametrize("grid", ["none", "invalid"])
@pytest.mark.parametrize("follow", [0, 2])
def test_unlit_one_without_maps_is_the_albedo_guide(api, follow, grid):
    """... and with a probe grid none of whose nodes is valid: the lookup's weights sum to 0 everywhere, it lights nothing, and the probe ending
    falls to unlit on every surface.  So the guides' ending, the baked one and the probe one leave the same bits"""
    r = api.Renderer(G.follow_room(), G.W, G.H, max_bounces=DEPTH)
    if grid == "invalid":
        sh = np.random.default_rng(25).uniform(1.0, 3.0, (2, 2, 2, 9, 3)).astype(F)      # bright wherever a node counted
        r.set_probe_grid((-10.0, -10.0, -10.0), (20.0, 20.0, 20.0), sh, valid=np.zeros((2, 2, 2), bool))
        assert r.probe_grid_info()[2] == (2, 2, 2) and r.probe_grid_info()[4] == 0
    for sample in (0, 5):
        got = _one(r, sample, follow, (1.0, 1.0, 1.0))
        r.render_guides(sample, follow=follow)
        surface = r.read_guides()[2] != MISS
        assert surface.sum() > 500 and (~surface).any()
        assert_bit_equal(got[surface], r.read_guide_albedo()[surface], f"sample {sample}, follow {follow}, grid {grid}")
        if follow:
            assert (r.read_guide_hops()[surface] > 0).any()


# ---- 3. chains that end at once as a miss or on a light are the path tracer's samples
@pytest.mark.parametrize("env", ["ambient", "environment"])
def test_first_hop_misses_and_lights_are_the_rendered_samples(api, env):
    sc = _room()["scene"]
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    if env == "environment":
        r.set_environment(np.random.default_rng(2).uniform(0.0, 4.0, (7, 12, 3)).astype(F))
    assert max(float(np.sqrt(sum(c * c for c in m.material.colour))) for m in sc.models if m.material.kind == EMISSIVE) < 100.0
    for sample in (0, 4):
        for follow in (0, 2):
            got = _one(r, sample, follow)                       # plain unlit: everything else is black
            r.render_guides(sample, follow=follow)
            model, hops = r.read_guides()[2], r.read_guide_hops()
            miss = (model == MISS) & (hops == 0)
            kinds = np.array([m.material.kind for m in sc.models])
            light = (model != MISS) & (hops == 0)
            light[light] = kinds[model[light] & 0x0FFFFFFF] == EMISSIVE
            assert miss.sum() > 100 and light.sum() > 5
            want = r.render_samples(sample, 1)[0][..., :3]
            assert_bit_equal(got[miss], want[miss], f"{env}: misses of sample {sample}")
            assert_bit_equal(got[light], want[light], f"{env}: lights of sample {sample}")
            if env == "environment":
                assert len(np.unique(got[miss][:, 0])) > 10
            else:
                assert (got[miss] == F(0.006)).all()
            other = ~miss & ~light & (hops == 0) & (model != MISS)
            assert not got[other].any()


# ---- 4. the mapped room against the oracle-walked chains
@pytest.mark.parametrize("follow", [0, 2])
def test_mapped_room_matches_the_restated_view(api, oracle_mod, follow):
    room = _room(oracle_mod)
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH)
    BC.set_maps(r, room["maps"])
    seen = set()
    for sample in (0, 3):
        want, ending = _want(oracle_mod, sample, follow)
        assert_bit_equal(_one(r, sample, follow, UNLIT), want, f"sample {sample}, follow {follow}")
        seen |= set(np.unique(ending).tolist())
        print(sample, follow, {BC.ENDINGS.get(k, "miss at once"): int((ending == k).sum()) for k in range(6)})
    needed = set(BC.ENDINGS) - ({BC.MISS_AFTER_HOPS} if follow == 0 else set())
    assert needed <= seen, (needed, seen)
    # the sums are the fold of the samples
    r.reset_baked()
    total = r.render_baked(0, 4, follow=follow, unlit=UNLIT)
    assert_bit_equal(total, BC.fold([_want(oracle_mod, s, follow)[0] for s in range(4)]), "four samples")
    assert_bit_equal(r.read_baked(), total, "pt_read_baked")


def test_mapped_room_on_a_rank(api, oracle_mod):
    room = _room(oracle_mod)
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH, rank=1, world_size=2, strip_rows=4)
    BC.set_maps(r, room["maps"])
    rows = r.local_rows().astype(np.int64)
    assert np.array_equal(rows, [4, 5, 6, 7, 12, 13, 14, 15])
    for follow in (0, 2):
        want, ending = _want(oracle_mod, 3, follow)
        assert_bit_equal(_one(r, 3, follow, UNLIT), want[rows], f"rank 1 of 2, follow {follow}")
        if follow:
            assert set(BC.ENDINGS) <= set(np.unique(ending[rows]).tolist())


# ---- 5. continuation and staleness
def test_sums_continue_and_restart(api):
    room = _room()
    sc = room["scene"]
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    BC.set_maps(r, room["maps"])
    whole = r.render_baked(0, 5, follow=2, unlit=UNLIT)
    r.reset_baked()
    r.render_baked(0, 3, follow=2, unlit=UNLIT)
    assert_bit_equal(r.render_baked(3, 2, follow=2, unlit=UNLIT), whole, "(0, 3) then (3, 2)")
    assert (whole[..., 3] == 5).all()

    def tail(**kw):
        """what (3, 2) gives now, onto five samples made with (follow 2, UNLIT): sums that went on would hold 5 + 2 samples"""
        base = dict(follow=2, unlit=UNLIT)
        got = r.render_baked(3, 2, **dict(base, **kw))
        assert (got[..., 3] == 2).all(), kw
        r.reset_baked()
        with pytest.raises(api.PtError):
            r.read_baked()                                                      # reset sums are no sums
        assert_bit_equal(r.render_baked(3, 2, **dict(base, **kw)), got, f"restart {kw}")
        r.reset_baked()
        r.render_baked(0, 5, **base)
        return got
    two = tail(follow=0)                                                        # another K
    assert not np.array_equal(two, tail(unlit=(0.25, 0.5, 0.25)))               # another unlit, even by one component
    name = BC.MAPPED_MODELS.index
    r.set_lightmap(name("back"), 0, room["maps"][name("tile"), 1])              # another map
    changed = tail()
    r.set_lightmap(name("back"), 0, room["maps"][name("back"), 0])
    back = tail()
    assert not np.array_equal(changed, back)
    r.set_camera(Camera.new((0.5, 0.0, 12.0), (0.0, -1.0, -2.0), 70.0, W / H))    # a camera move
    assert not np.array_equal(tail(), back)
    r.rebuild()                                                                 # pt_build keeps the maps and restarts the sums
    r.set_camera(sc.camera)
    assert_bit_equal(tail(), back, "after a rebuild the maps are still there")
    # an unchanged call continues
    assert (r.render_baked(5, 1, follow=2, unlit=UNLIT)[..., 3] == 6).all()


# ---- 6. isolation
def test_the_view_leaves_frame_moments_and_guides_alone(api):
    room = _room()
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    r.render(0, 3)
    launches = r.last_launches()
    r.render_guides(1, follow=2)

    def state():
        pos, nrm, model = r.read_guides()
        return r.read_frame() + (r.read_moments(), pos, nrm, model, r.read_guide_instances(), r.read_guide_albedo(), r.read_guide_hops())
    before, info = state(), r.scene_info().as_dict()
    BC.set_maps(r, room["maps"])
    r.render_baked(0, 2, follow=8, unlit=UNLIT)
    r.render_baked(2, 1, follow=0)
    for a, b in zip(before, state()):
        assert_bit_equal(a, b, "frame, moments and guides")
    filtered = r.denoise()                                                      # the guides are still current
    assert np.isfinite(filtered).all()
    # a refused call leaves the sums as they are
    kept = r.read_baked()
    assert r.L.pt_render_baked(r.ctx, 0, 1, C.byref(api.BakedParams(9)), None) == -1
    assert r.L.pt_render_baked(r.ctx, 0, 0, C.byref(api.BakedParams(0)), None) == -1
    assert_bit_equal(r.read_baked(), kept, "sums after refused calls")
    # a scene with lightmaps renders with the launches it had, and is no textured scene
    assert r.scene_info().as_dict() == info
    r.reset_accumulation()
    r.render(0, 3)
    assert r.last_launches() == launches
    for a, b in zip(before[:4], r.read_frame() + (r.read_moments(),)):
        assert_bit_equal(a, b, "the render after pt_set_lightmap")


# ---- 7. the C++ surface
def test_headless_baked_view_matches_the_python_route(api, tmp_path):
    """examples/headless --bake-lightmap 16 16 8 2 map.txt --baked-view 3 view.png: the map it bakes, set as sum / 8 on the shell, shown"""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_post import _read_png
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, BOUNCES = 48, 32, 4
    exe = B.build_host_driver()
    png = tmp_path / "view.png"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES), "--bake-lightmap", "16", "16", "8", "2",
                          str(tmp_path / "map.txt"), "--baked-view", "3", str(png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    refused = subprocess.run([exe, "--baked-view", "3", str(png)], capture_output=True, text=True, cwd=ROOT)
    assert refused.returncode == 2 and "--bake-lightmap" in refused.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    p = r.model_vertices(1)[0].reshape(-1, 3)[:, [0, 2]]
    lo, hi = p.min(0), p.max(0)
    r.set_model_uvs(1, ((p - lo) / (hi - lo)).astype(F).reshape(-1, 3, 2))
    r.rebuild()
    sums, cov = r.dilate_lightmap(*r.bake_lightmap(1, 0, 16, 16, 8, bias=0.25), 2)
    r.set_lightmap_sums(1, 0, sums, 8)
    view = r.render_baked(0, 3)
    got = _read_png(png)
    assert np.array_equal(got, r.post_rgb8(view))
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 50                      # a picture, not a flat frame
    r.write_baked_image(tmp_path / "again.png")
    assert np.array_equal(_read_png(tmp_path / "again.png"), got)


# ---- 8. the picture means what the bake means
def test_baked_view_agrees_with_the_path_traced_frame(api):
    """A closed Lambertian room, every placement baked at 48 x 32 texels with max_bounces = B, dilated twice, set as sum / n; the baked view
    (16 samples, K = 0) against pt_render of the same frame at max_bounces = B + 1 (a baked ray starts one bounce later).  The statistic is
    the relative difference of the two frame-mean luminances; the same statistic between two path-traced frames of different seeds is the
    noise floor, printed beside it.  The bound of 10 % is set by what the test has to catch: a dropped albedo of 0.7 is 43 %, a stray pi
    214 %.  Measured on an MI355X: see profiles/r22_baked_view.md."""
    Wd, Hd, B, SPP, BAKE = 48, 32, 3, 16, 64
    sc, placements = BC.lit_room(Wd, Hd)
    r = api.Renderer(sc, Wd, Hd, max_bounces=B)
    for model, ordinal in placements:
        sums, cov = r.bake_lightmap(model, ordinal, 48, 32, BAKE, bias=0.01)
        assert cov.sum() > 500
        sums, cov = r.dilate_lightmap(sums, cov, passes=2)
        r.set_lightmap_sums(model, ordinal, sums, BAKE)
    view = r.render_baked(0, SPP)
    r.render_guides(0)
    assert (r.read_guides()[2] != MISS).all()                                   # every first hit is a surface

    def traced(seed):
        p = api.Renderer(sc, Wd, Hd, max_bounces=B + 1, seed=seed)
        acc = p.render(0, SPP, want_position=False)[0]
        return float(BC.luminance(acc[..., :3] / acc[..., 3:4]).mean())
    baked = float(BC.luminance(view[..., :3] / view[..., 3:4]).mean())
    a, b = traced(api.DEFAULT_SEED), traced(12345)
    diff, floor = abs(baked - a) / a, abs(b - a) / a
    print(f"baked view: mean luminance {baked:.5f}, path traced {a:.5f} (seed 2: {b:.5f}); relative difference {diff:.4f}, noise floor {floor:.4f}")
    assert diff < 0.10
