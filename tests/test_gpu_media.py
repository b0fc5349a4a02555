"""GPU (-m gpu): participating media at the volume stack's edges, against the CPU oracle (bit-exact) and, where the oracle's own
semantics are in question, against a property that needs no oracle.  The stack (integrator.rs:161,189-227) holds up to eight
volumes per path on the device, keyed per model as the reference keys them; the oracle's is unbounded."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_oracle_kat import VOLUME_CASES, _stream_f32, check_volume_eval, volume_eval_inputs, volume_probe_scene

pytestmark = pytest.mark.gpu
W, H = 48, 32


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _okw(kw):
    return {k: (int(v) if k == "enable_nee" else v) for k, v in kw.items()}


def _parity(api, oracle_mod, sc, spp=3, min_depth=None, depth=None, **kw):
    """per-sample radiance, the frame (accumulation, position, id history) and the ray tallies against the oracle; returns the
    oracle's deepest volume stack (counter 8) after checking that the scene reaches the depth the caller wants to test"""
    o = oracle_mod.Oracle(sc)
    oacc, opos, oid, octr = o.render(W, H, spp, **_okw(kw))
    if depth is not None:
        assert int(octr[8]) == depth, ("the scene does not reach the depth under test", int(octr[8]))
    if min_depth is not None:
        assert int(octr[8]) >= min_depth, ("the scene does not reach the depth under test", int(octr[8]))
    r = api.Renderer(sc, W, H, **kw)
    assert_bit_equal(r.render_samples(0, spp), o.render_samples(W, H, spp, **_okw(kw)), f"{sc.name} {kw} per-sample radiance")
    r.reset_stats()
    acc, pos, idb = r.render(0, spp)
    assert_bit_equal(acc, oacc, f"{sc.name} frame"); assert_bit_equal(pos, opos, f"{sc.name} position"); assert np.array_equal(idb, oid)
    st = r.stats()
    assert (st.rays_closest, st.rays_any, st.rays_light_closest) == (int(octr[0]), int(octr[1]), int(octr[2]))
    return int(octr[8])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_nested_volumes_up_to_the_stack_depth(api, oracle_mod, n):
    from path_tracer_amd import scenes
    _parity(api, oracle_mod, scenes.media_shells(n), depth=n, max_bounces=12)


def test_ninth_nested_volume_is_an_error_not_dropped(api, oracle_mod):
    """a path inside nine volumes cannot be held: the render fails with PT_ERR_LIMIT naming the volume stack, leaves the
    accumulation reset, and the context renders correctly again once no path gets that deep"""
    from path_tracer_amd import scenes
    sc = scenes.media_shells(9)
    o = oracle_mod.Oracle(sc)
    assert int(o.render(W, H, 3, max_bounces=12)[3][8]) == 9
    r = api.Renderer(sc, W, H, max_bounces=12)
    with pytest.raises(api.PtError) as e:
        r.render(0, 3)
    assert e.value.code == -5 and "volume" in str(e.value)
    assert not r.read_accumulation().any(), "a failed render leaves the accumulation reset"
    # at 4 bounces no path is inside more than five shells
    oacc, _, _, octr = o.render(W, H, 3, max_bounces=4)
    assert int(octr[8]) <= 8
    r.set_config(max_bounces=4)
    r.reset_accumulation()
    assert_bit_equal(r.render(0, 3)[0], oacc, "same context after the volume-stack error")
    # and a neighbouring context without volumes is unharmed
    cb = scenes.cornell_box(W, H)
    assert_bit_equal(api.Renderer(cb, W, H, max_bounces=5).render(0, 2)[0], oracle_mod.Oracle(cb).render(W, H, 2, max_bounces=5)[0], "no volumes")


def test_leaving_a_volume_from_the_middle_of_the_stack(api, oracle_mod):
    """enter A, B, C, leave B: the RNG draws of the media loop follow the stack order, so only bit equality shows that the gap is
    closed in insertion order"""
    from path_tracer_amd import scenes
    _parity(api, oracle_mod, scenes.media_chain(W, H), spp=4, min_depth=3, max_bounces=10)


@pytest.mark.parametrize("variant,depth", [("a", 2), ("b", 1), ("c", 1)])
def test_volume_identity_is_per_model(api, oracle_mod, variant, depth):
    """(a) two models of one absorbing glass: two volumes; (b) two instances of one model and (c) one model with both spheres: one"""
    from path_tracer_amd import scenes
    _parity(api, oracle_mod, scenes.media_pair(variant, W, H), spp=4, depth=depth, max_bounces=8)


def test_two_models_of_one_material_absorb_twice_without_the_oracle(api):
    """Scenes (a) and (c) with absorption only and max_bounces=3 trace the same paths: Russian roulette starts at b > 3
    (integrator.rs:166) and absorption draws nothing.  In (a) a path is inside one volume per sphere, in (c) inside at most one:
    every radiance of (a) is <= that of (c), strictly smaller somewhere, and the ray tallies are equal."""
    from path_tracer_amd import scenes
    out, tallies = {}, {}
    for v in ("a", "c"):
        r = api.Renderer(scenes.media_pair(v, W, H), W, H, max_bounces=3)
        r.reset_stats()
        out[v] = r.render_samples(0, 6)[..., :3]
        st = r.stats()
        tallies[v] = (st.rays_closest, st.rays_any, st.rays_light_closest)
    assert tallies["a"] == tallies["c"]
    assert np.isfinite(out["c"]).all() and np.linalg.norm(out["c"].astype(np.float64), axis=-1).max() <= 100.0, "clamp_length_max(100) never rescales"
    assert (out["a"] <= out["c"]).all()
    assert (out["a"] < out["c"]).any()


def test_camera_inside_a_volume(api, oracle_mod):
    """the first hit is a back face of a sphere whose volume the path never entered: leaving it does nothing"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Dielectric, Model, Volume
    t, n = scenes.sphere_mesh(2, (0.0, 50.0, 900.0), 220.0)
    around = Model.new(t.astype(np.float32), n.astype(np.float32), Dielectric.new((0.99, 0.99, 0.99), 1.1, Volume.new((0.5, 0.3, 0.1), 0.003, 1.0 / 400.0, 0.5)))
    t2, n2 = scenes.sphere_mesh(2, (0.0, 0.0, 0.0), 120.0)
    inner = Model.new(t2.astype(np.float32), n2.astype(np.float32), Dielectric.new((0.95, 0.95, 0.95), 1.3, Volume.new((0.1, 0.6, 0.9), 0.01, 1.0 / 150.0, -0.3)))
    _parity(api, oracle_mod, scenes.media_room(W, H, [around, inner], "camera_inside"), spp=4, min_depth=1, max_bounces=8)


@pytest.mark.parametrize("enable_nee", [True, False])
def test_every_shading_class_inside_a_medium(api, oracle_mod, enable_nee):
    """Lambertian, specular, GGX metal, GGX dielectric, smooth dielectric and an emitter inside one scattering sphere: every
    k_shade_surface<., VOLUMES=true> instance, and emissive hits shaded by the Lambert class"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import GGX, Dielectric, Emissive, Lambertian, Model, Specular, Volume
    def sph(c, r, m, lvl=1):
        t, n = scenes.sphere_mesh(lvl, c, r)
        return Model.new(t.astype(np.float32), n.astype(np.float32), m)
    models = [sph((0.0, 30.0, 0.0), 250.0, Dielectric.new((1.0, 1.0, 1.0), 1.01, Volume.new((0.2, 0.4, 0.6), 0.001, 1.0 / 250.0, 0.2)), 2),
              sph((-120.0, 0.0, 0.0), 50.0, Lambertian.new((0.7, 0.6, 0.5))),
              sph((0.0, 0.0, 0.0), 45.0, Specular.new((0.9, 0.9, 0.9))),
              sph((120.0, 0.0, 0.0), 50.0, GGX.new_metal((0.9, 0.6, 0.2), 0.3)),
              sph((-60.0, 110.0, 40.0), 40.0, GGX.new_dielectric((0.95, 0.95, 0.95), 0.2, 1.5, Volume.new((0.0, 0.0, 0.0), 0.0, 1.0 / 30.0, 0.0))),
              sph((60.0, 110.0, 40.0), 40.0, Dielectric.new((0.95, 0.95, 0.95), 1.5, None)),
              sph((0.0, -90.0, 80.0), 25.0, Emissive.new((8.0, 6.0, 4.0)))]
    _parity(api, oracle_mod, scenes.media_room(W, H, models, "classes_in_medium"), spp=4, min_depth=1, max_bounces=8, enable_nee=enable_nee)


@pytest.mark.parametrize("absorption,k,c,g", [
    ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, 0.999), ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, -0.999),
    ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, 1.0), ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, -1.0),
    ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, 5.0), ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, -5.0),
    ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, 0.0), ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, -0.0), ((0.4, 0.6, 0.7), 0.01, 1.0 / 60.0, 1e-30),
    ((0.0, 0.0, 0.0), 0.0, 1.0, 0.3),          # dense: every segment scatters
    ((0.0, 0.0, 0.0), 0.0, 1e-7, 0.3),         # thin: nearly never
    ((0.45, 0.5, 0.55), 1.0, 0.0, 0.0),        # transmissions down in the denormals
    ((0.5, 0.6, 0.7), 1e30, 0.0, 0.0),         # huge k: transmission 0 through any length
    ((0.0, 0.5, 1.0), 0.05, 1.0 / 80.0, 0.6),  # an absorption colour with a zero channel
])
def test_volume_parameter_edges(api, oracle_mod, absorption, k, c, g):
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Dielectric, Model, Volume
    t, n = scenes.sphere_mesh(2, (0.0, 20.0, 0.0), 140.0)
    m = Model.new(t.astype(np.float32), n.astype(np.float32), Dielectric.new((0.98, 0.98, 0.98), 1.2, Volume.new(absorption, k, c, g)))
    _parity(api, oracle_mod, scenes.media_room(W, H, [m], "edge"), spp=3, depth=1, max_bounces=8)


def test_media_batch_structure_does_not_change_the_image(api, oracle_mod):
    """the per-path stack lives in each pipeline's pool, is indexed by path id and is reset at bounce 0 only"""
    from path_tracer_amd import scenes
    from path_tracer_amd.dist import rows_of_rank
    sc = scenes.media_chain(W, H)
    kw = dict(max_bounces=8)
    want = oracle_mod.Oracle(sc).render(W, H, 6, **kw)[0]
    ref = api.Renderer(sc, W, H, **kw).render(0, 6)
    assert_bit_equal(ref[0], want, "vs oracle")
    for cfg in (dict(batch_spp=1), dict(batch_spp=2, pipelines=2), dict(flags=2)):
        assert_bit_equal(api.Renderer(sc, W, H, **kw, **cfg).render(0, 6)[0], want, str(cfg))
    res = api.Renderer(sc, W, H, batch_spp=4, **kw)
    idb = np.zeros((H, W), np.uint32)
    res.render(0, 4, ident=idb)
    assert_bit_equal(res.render(4, 2, ident=idb)[0], want, "resumed at first_sample=4")
    full = np.zeros_like(want)
    for rank in range(3):
        rr = api.Renderer(sc, W, H, rank=rank, world_size=3, strip_rows=4, **kw)
        full[rows_of_rank(H, rank, 3, 4)] = rr.render(0, 6)[0]
    assert_bit_equal(full, want, "three row-sharded ranks")


def test_scene_edit_adds_the_first_volume(api, oracle_mod):
    """a context whose pool was sized without volume stacks gets one when a rebuilt scene has volumes (ensure_wavefront's vstack_ok)"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import SceneDesc
    base = scenes.cornell_box(W, H)
    r = api.Renderer(base, W, H, max_bounces=6)
    r.render(0, 2)
    extra = scenes.media_pair("a").models[-2:]
    for m in extra:
        r.add_model(m)
    r.rebuild()
    sc2 = SceneDesc.new(list(base.models) + list(extra), base.camera, "edited")
    assert_bit_equal(r.render_samples(0, 3), oracle_mod.Oracle(sc2).render_samples(W, H, 3, max_bounces=6), "after adding two volume models")


@pytest.mark.parametrize("g,c,k", VOLUME_CASES)
def test_volume_eval_matches_oracle_and_binary64(api, oracle_mod, g, c, k):
    """pt_volume_eval (the shading pass's media arithmetic) against pto_volume_eval bit for bit, and both against binary64"""
    from path_tracer_amd.scene_desc import Volume
    vol = Volume.new((0.4, 0.0, 0.9), k, c, g)
    sc = volume_probe_scene(vol)
    r = api.Renderer(sc, 8, 8)
    o = oracle_mod.Oracle(sc)
    mi = len(sc.materials()) - 1
    inc, t_max, dist, px, sm = volume_eval_inputs(12000, 11)
    g_out = r.volume_eval(mi, inc, t_max, dist, px, sm, 2)
    o_out = np.stack([o.volume_eval(mi, inc[i], t_max[i], dist[i], int(px[i]), int(sm[i]), 2) for i in range(len(px))])
    assert_bit_equal(g_out, o_out, f"volume_eval g={g}")
    L = oracle_mod.lib()
    u = np.array([[_stream_f32(L, oracle_mod.DEFAULT_SEED, px[i], sm[i], 2 + j) for j in range(3)] for i in range(len(px))], np.float64)
    check_volume_eval(g_out, vol, inc, t_max, dist, u[:, 0], u[:, 1], u[:, 2])


@pytest.mark.parametrize("g", [-0.6, 0.0, 0.6, 0.95])
def test_henyey_greenstein_mean_cosine(api, g):
    """over 10^6 draws the mean of z (measured along -incoming: the reference builds its ONB on -incoming, volume.rs:59) is the HG
    mean cosine g, within 5 sigma"""
    from path_tracer_amd.scene_desc import Volume
    vol = Volume.new((0.0, 0.0, 0.0), 0.0, 1.0, g)
    sc = volume_probe_scene(vol)
    r = api.Renderer(sc, 8, 8)
    n = 1 << 20
    rng = np.random.default_rng(5)
    inc = rng.normal(size=(n, 3))
    inc = (inc / np.linalg.norm(inc, axis=1, keepdims=True)).astype(np.float32)
    out = r.volume_eval(len(sc.materials()) - 1, inc, np.full(n, np.inf, np.float32), np.zeros(n, np.float32),
                        np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), 0)
    assert (out[:, 0] == 1.0).all()
    z = (out[:, 2:5].astype(np.float64) * -inc.astype(np.float64)).sum(1)
    z = z[np.isfinite(z)]
    sigma = z.std() / np.sqrt(z.size)
    assert abs(z.mean() - g) < 5 * sigma + 1e-6, (z.mean(), g, sigma)
