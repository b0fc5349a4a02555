"""GPU: the ray-claim and queue-region arithmetic (pt_queue_plan.h) under the real kernels, at the ray counts where a regime changes:
below, on and above a wave, a workgroup, the launch's lanes, every power of two up to 2^21 (the static / dynamic split, the tapered
chunk levels, the striped tails' log_k steps from 2^15 to 2^20).  A lost ray, one traced twice, a hit record the shading pass skips or a
slot read that nobody wrote changes a result or a tally.

The reference is the CPU oracle on a TILE of 997 rays, independent of the code under test: ray i of a call with n rays is tile ray
i % 997, so row i of the expected result is the oracle's row i % 997.  997 is prime: the tile never lines up with a chunk.  The
workgroup shape each scene runs with is asserted (pt_trace_geometry), so that a later change of a scene or a threshold cannot silently
empty a case.  (The 64-thread shape needs more than 24 stack levels in LDS; no scene here is that deep, tests/test_queue_plan_host.py
covers one wave per workgroup on the host.)"""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
M = 997
DEPTH = 4
SMALL = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def _pow2(k0, k1):
    return [(1 << k) + d for k in range(k0, k1 + 1) for d in (-1, 0, 1)]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _tile():
    """the rays of test_gpu_parity.test_trace_matches_oracle_on_random_rays, 997 of them: random ones, axis-aligned directions, origins on the
    room's and the boxes' planes, signed-zero direction components on such a plane's axis; t_max with NaN, inf and 0 among them; stream keys over
    all 32 bits"""
    rng = np.random.default_rng(3)
    n = M
    O = rng.uniform(-270, 270, (n, 3)).astype(F)
    O[:, 1] += 50
    D = rng.normal(size=(n, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F)
    D[:300] = np.eye(3, dtype=F)[rng.integers(0, 3, 300)] * rng.choice([-1.0, 1.0], (300, 1)).astype(F)
    O[300:400] = np.round(O[300:400] / 139) * 139
    D[400:420, 2] = -0.0
    D[400:420] /= np.linalg.norm(D[400:420], axis=1, keepdims=True)
    planes = np.array([-278.0, 278.0, -228.0, 328.0, 0.0, 139.0, -139.0], F)
    for i in range(420, 720):
        ax = int(rng.integers(0, 3))
        O[i, ax] = planes[rng.integers(0, len(planes))]
        D[i, ax] = rng.choice(np.array([0.0, -0.0], F))
        if i % 3 == 0:
            D[i, (ax + 1) % 3] = rng.choice(np.array([0.0, -0.0], F))
        D[i] = (D[i] / np.linalg.norm(D[i].astype(np.float64))).astype(F)
    tm = rng.uniform(0, 800, n).astype(F)
    tm[:50] = np.nan
    tm[50:100] = np.inf
    tm[100:120] = 0.0
    key = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    sample = rng.integers(0, 2000, n).astype(np.uint32)
    return O, D, tm, key, sample


TILE = _tile()


def _scene(name):
    from path_tracer_amd import scenes
    return {"box": lambda: scenes.cornell_box(64, 64), "mesh2": lambda: scenes.cornell_mesh(64, 64, level=2), "mixed": lambda: scenes.cornell_mixed(64, 64)}[name]()


def _env():
    return (np.random.default_rng(21).uniform(0, 1, (17, 33, 3)) ** 3 * 4).astype(F)


# name: scene, Renderer keywords, expected {block_threads, BVH in LDS, stack levels spilled, shadow rays walked inside the shading pass}
HOOK_CASES = {
    "box_lds_256": ("box", dict(), dict(block_threads=256, lds=True, spill=False, inline_shadow=True)),
    "mesh2_lds_128": ("mesh2", dict(), dict(block_threads=128, lds=True, spill=False, inline_shadow=False)),
    "box_global": ("box", dict(flags=2), dict(block_threads=256, lds=False, spill=False, inline_shadow=False)),      # PT_FLAG_NO_LDS_SCENE: chunk divisor 16
    "mesh2_spill": ("mesh2", dict(stack_lds_levels=2), dict(block_threads=256, lds=True, spill=True, inline_shadow=False)),
}
INTEGRATE_CASES = {
    "mixed": ("mixed", dict(), False, dict(block_threads=256, lds=True, spill=False, inline_shadow=True)),
    "mixed_env": ("mixed", dict(), True, dict(block_threads=256, lds=True, spill=False, inline_shadow=True)),        # every miss goes through the terminal queue
    "mixed_global": ("mixed", dict(flags=2), False, dict(block_threads=256, lds=False, spill=False, inline_shadow=False)),  # queued shadow rays
}
_RENDERERS, _ORACLES, _EXPECT = {}, {}, {}


def _renderer(api, case, table):
    if case not in _RENDERERS:
        spec = table[case]
        r = api.Renderer(_scene(spec[0]), 64, 64, max_bounces=DEPTH, **spec[1])
        if table is INTEGRATE_CASES and spec[2]:
            r.set_environment(_env())
        geo = r.trace_geometry()
        st = r.stats()
        want = spec[-1]
        got = dict(block_threads=geo["block_threads"], lds=bool(st.lds_scene), spill=st.stack_entries > geo["stack_lds"], inline_shadow=geo["shade_traces_shadow"])
        print(f"{case}: geometry {geo}, lds_scene {st.lds_scene}, stack_entries {st.stack_entries}, scene_bytes {st.scene_bytes}")
        assert got == want, (case, geo, got, want)
        assert geo["trace_blocks"] >= 256 and (want["spill"] is False or geo["stack_lds"] == 2), (case, geo)
        _RENDERERS[case] = (r, geo)
    return _RENDERERS[case]


def _oracle(oracle_mod, scene, env=False):
    if (scene, env) not in _ORACLES:
        o = oracle_mod.Oracle(_scene(scene))
        if env:
            o.set_environment(_env())
        _ORACLES[(scene, env)] = o
    return _ORACLES[(scene, env)]


def _lane_counts(geo):
    lanes = geo["trace_blocks"] * geo["block_threads"]
    return [lanes - 1, lanes, lanes + 1, 4 * lanes + 1]


def _index(n):
    return np.arange(n) % M


# ---- the trace hooks
HOOKS = ["closest_world", "closest_lights", "closest_world_tmax", "closest_lights_tmax", "any_world", "any_lights"]


def _hook(obj, hook, O, D, tm):
    which = 1 if "lights" in hook else 0
    if hook.startswith("any"):
        return {"hit": obj.trace_any(O, D, tm, which=which)}
    h = obj.trace_closest(O, D, tm if hook.endswith("tmax") else None, which=which)
    return {k: h[k] for k in ("inst", "prim", "t", "u", "v")}


@pytest.mark.parametrize("hook", HOOKS)
@pytest.mark.parametrize("case", list(HOOK_CASES))
def test_trace_hooks_at_every_ray_count(api, oracle_mod, case, hook):
    r, geo = _renderer(api, case, HOOK_CASES)
    scene = HOOK_CASES[case][0]
    O, D, tm, _, _ = TILE
    if (scene, hook) not in _EXPECT:
        _EXPECT[(scene, hook)] = _hook(_oracle(oracle_mod, scene), hook, O, D, tm)
    want = _EXPECT[(scene, hook)]
    some = want["hit"] if "hit" in want else want["inst"] != 0xffffffff
    assert some.any() and not some.all(), "the tile holds hits and misses"
    for n in sorted(set(SMALL + _pow2(12, 21) + _lane_counts(geo))):
        idx = _index(n)
        got = _hook(r, hook, O[idx], D[idx], tm[idx])
        for k, w in want.items():
            assert_bit_equal(got[k], w[idx], f"{case} {hook} n={n}: {k}")


# ---- the integrator: the shade queues' striped tails step at every power of two from 2^15 to 2^20
INTEGRATE_COUNTS = [1, 63, 64, 65, 257] + _pow2(15, 20)


@pytest.mark.parametrize("case", list(INTEGRATE_CASES))
def test_integrated_rays_at_every_ray_count(api, oracle_mod, case):
    r, geo = _renderer(api, case, INTEGRATE_CASES)
    scene, _, env, _ = INTEGRATE_CASES[case]
    O, D, _, key, sample = TILE
    if ("integrate", scene, env) not in _EXPECT:
        _EXPECT[("integrate", scene, env)] = _oracle(oracle_mod, scene, env).integrate_counted(O, D, key, sample, 1, max_bounces=DEPTH)
    rad, pos, idb, casts = _EXPECT[("integrate", scene, env)]
    assert (idb == 255).any() and (idb != 255).any() and casts[:, 1].any() and casts[:, 2].any(), "the tile has misses, hits, shadow rays and light-sampled rays"
    for n in INTEGRATE_COUNTS:
        idx = _index(n)
        r.reset_stats()
        g = r.integrate_rays(O[idx], D[idx], key[idx], sample[idx])
        assert_bit_equal(g[0], rad[idx], f"{case} n={n}: radiance")
        assert_bit_equal(g[1], pos[idx], f"{case} n={n}: first hit")
        assert np.array_equal(g[2], idb[idx]), f"{case} n={n}: id"
        st = r.stats()
        tally = (n // M) * casts.sum(0) + casts[: n % M].sum(0)     # whole tiles and the remainder's share
        assert (st.rays_closest, st.rays_any, st.rays_light_closest) == tuple(int(v) for v in tally), (case, n, st.as_dict(), tally)


# ---- frames at awkward shapes
SHAPES = [(1, 1), (1, 7), (7, 1), (1, 257), (257, 1), (3, 5), (63, 1), (65, 3), (127, 2)]     # width x height
SPP = (1, 3, 17)
CAMERAS = {"reference": None, "corner": ((900.0, 700.0, 1100.0), (0.0, 0.0, 0.0), 35.0)}    # None: the scene's own pinhole; "corner": the box's image is a hexagon


def _frame_scene(camera, w, h):
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Camera, SceneDesc
    if CAMERAS[camera] is None:
        return scenes.cornell_box(w, h)
    eye, target, fov = CAMERAS[camera]
    return SceneDesc.new(scenes.cornell_models(), Camera.new(eye, target, fov, w / h), "view")


def _tallies(st):
    return np.array([st.rays_closest, st.rays_any, st.rays_light_closest], np.uint64)


@pytest.mark.parametrize("camera", list(CAMERAS))
def test_frames_at_awkward_shapes(api, oracle_mod, camera):
    """accumulation, first-hit position, id history and the three ray tallies of whole frames; 17 samples make two blocks of path ids, the
    last one a single sample"""
    subset = []
    for w, h in SHAPES:
        sc = _frame_scene(camera, w, h)
        r = api.Renderer(sc, w, h, max_bounces=DEPTH)
        o = oracle_mod.Oracle(sc)
        for spp in SPP:
            r.reset_accumulation()
            r.reset_stats()
            acc, pos, idb = r.render(0, spp)
            oacc, opos, oid, octr = o.render(w, h, spp, max_bounces=DEPTH)
            assert_bit_equal(acc, oacc, f"{camera} {w} x {h}, {spp} spp: accumulation")
            assert_bit_equal(pos, opos, f"{camera} {w} x {h}, {spp} spp: position")
            assert np.array_equal(idb, oid), f"{camera} {w} x {h}, {spp} spp: id"
            assert np.array_equal(_tallies(r.stats()), octr[:3]), (camera, w, h, spp, r.stats().as_dict(), octr)
        (x0, aw, y0, ah), _ = r.active_pixels()
        assert aw <= w and ah <= h
        subset.append(aw * ah < w * h)
        r.close()
    print(f"{camera}: active rectangle a strict subset at {[s for s, f in zip(SHAPES, subset) if f]}")
    if camera == "corner":
        assert any(subset), "this camera is here for frames whose active rectangle leaves pixels out"


@pytest.mark.parametrize("strip_rows", [1, 2])
@pytest.mark.parametrize("w,h", [(65, 3), (127, 2)])
def test_sharded_frames_at_awkward_shapes(api, oracle_mod, w, h, strip_rows):
    """three ranks over two or three rows: some ranks own one row, some none; the strips reassemble to the oracle's frame and the ranks'
    tallies add up to its"""
    from path_tracer_amd.dist import rows_of_rank
    rows = [rows_of_rank(h, rank, 3, strip_rows) for rank in range(3)]
    assert any(len(x) <= 1 for x in rows), rows
    for camera in CAMERAS:
        sc = _frame_scene(camera, w, h)
        o = oracle_mod.Oracle(sc)
        ranks = [api.Renderer(sc, w, h, max_bounces=DEPTH, rank=rank, world_size=3, strip_rows=strip_rows) for rank in range(3)]
        for spp in SPP:
            acc = np.zeros((h, w, 4), F); pos = np.zeros((h, w, 4), F); idb = np.zeros((h, w), np.uint32)
            tally = np.zeros(3, np.uint64)
            for rr, mine in zip(ranks, rows):
                rr.reset_accumulation()
                rr.reset_stats()
                a, p, i = rr.render(0, spp)
                assert a.shape == (len(mine), w, 4)
                acc[mine], pos[mine], idb[mine] = a, p, i
                tally += _tallies(rr.stats())
            oacc, opos, oid, octr = o.render(w, h, spp, max_bounces=DEPTH)
            assert_bit_equal(acc, oacc, f"{camera} {w} x {h} strips of {strip_rows}, {spp} spp: accumulation")
            assert_bit_equal(pos, opos, f"{camera} {w} x {h} strips of {strip_rows}, {spp} spp: position")
            assert np.array_equal(idb, oid), f"{camera} {w} x {h} strips of {strip_rows}, {spp} spp: id"
            assert np.array_equal(tally, octr[:3]), (camera, w, h, strip_rows, spp, tally, octr)
        for rr in ranks:
            rr.close()
