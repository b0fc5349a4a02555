"""GPU (-m gpu): pt_set_config on a live context, held to the contract include/pt_api.h states at pt_set_config.
 1. one context led through the walk of tests/reconfig_common.py: at every step every product is a fresh context's bit for bit, the render
    is the oracle's on the step's local rows, and a flag that only changes the route really changed it (pt_last_launches);
 2. a change of the SET of local pixels that keeps their number (32 x 24 -> 24 x 32, rank 0 -> 1 of 2, strip_rows 4 -> 2) drops the frame
    state like any other;
 3. a change that keeps the set keeps accumulation, moments and temporal history, and makes guides, albedo and baked sums stale;
 4. a refused call on a live context changes nothing;
 5. the pipelines' pools and the resident scene follow the configuration.
Everything is bit-exact.  Frames are 40 x 24 at the most, 3 samples, depth <= 6."""
import numpy as np
import pytest

import baked_common as BC
import reconfig_common as RC
from conftest import assert_bit_equal
from reconfig_common import ERR_STATE, M

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_ORACLE = {}


def _oracle(O):
    if "o" not in _ORACLE:
        _ORACLE["o"] = O.Oracle(RC.scene())
    return _ORACLE["o"]


def _oracle_render(O, cfg, n=M, first_sample=0):
    """the oracle's frame of a configuration (made once per distinct one, left unchanged), on the configuration's local rows; its ray tallies
    count the whole frame"""
    key = (cfg["width"], cfg["height"], cfg["max_bounces"], cfg["n_sobol"], cfg["seed"], cfg["enable_nee"], n, first_sample)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(O).render(cfg["width"], cfg["height"], n, first_sample=first_sample, max_bounces=cfg["max_bounces"],
                                         n_sobol=cfg["n_sobol"], seed=cfg["seed"], enable_nee=cfg["enable_nee"])
    return _ORACLE[key]


def _same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert_bit_equal(a[k], b[k], f"{what}: {k}")


def _raises_state(api, call, what):
    with pytest.raises(api.PtError) as e:
        call()
    assert e.value.code == ERR_STATE, (what, e.value.code)


def _zero(a, what):
    assert not np.ascontiguousarray(a).view(np.uint8).any(), what


# ------------------------------------------------------------------------------------------------------ 1. walked = fresh = oracle
CHUNKS = [(1, 7), (7, 14), (14, 20), (20, 25), (25, 30)]
assert CHUNKS[0][0] == 1 and CHUNKS[-1][1] == len(RC.WALK) and all(a[1] == b[0] for a, b in zip(CHUNKS, CHUNKS[1:]))


def _check_step(api, O, r, i, cfg, prev_routes):
    kind, change = RC.WALK[i]
    what = f"step {i} ({kind} {change})"
    got, routes = RC.products(api, r, cfg)
    fresh = RC.renderer(api, cfg)
    want, fresh_routes = RC.products(api, fresh, cfg)
    fresh.close()
    _same(got, want, what)
    assert routes == fresh_routes, (what, routes, fresh_routes)
    # the route the configuration asks for, taken by the walked context
    assert routes["bvh"] == {0 if cfg["flags"] & RC.FLAG_NO_LDS_SCENE else 1}, (what, routes)
    assert routes["spill"] == {1 if cfg["stack_lds_levels"] == RC.SPILL_LEVELS else 0}, (what, routes)
    assert routes["lights_ident"] == {0 if cfg["flags"] & RC.FLAG_GENERAL_WALK else 1}, (what, routes)
    if i:
        prev = RC.configs()[i - 1]
        if prev["stack_lds_levels"] != cfg["stack_lds_levels"] or (prev["flags"] ^ cfg["flags"]) & (RC.FLAG_NO_LDS_SCENE | RC.FLAG_GENERAL_WALK):
            assert routes != prev_routes, (what, "the step changed no route", routes)
    # the fresh context is code under test too: the render against the oracle, on the local rows
    rows = RC.model_rows(cfg)
    oacc, opos, oid, octr = _oracle_render(O, cfg)
    assert_bit_equal(got["accumulation"], oacc[rows], what + ": accumulation against the oracle")
    assert_bit_equal(got["position"], opos[rows], what + ": position against the oracle")
    assert np.array_equal(got["id"], oid[rows]), what + ": id history against the oracle"
    assert_bit_equal(got["render_samples"], _oracle(O).render_samples(cfg["width"], cfg["height"], M, max_bounces=cfg["max_bounces"], n_sobol=cfg["n_sobol"],
                                                                     seed=cfg["seed"], enable_nee=cfg["enable_nee"])[:, rows], what + ": per-sample radiance against the oracle")
    if (cfg["world_size"] or 1) == 1:
        assert tuple(int(x) for x in got["tallies of the render"][:3]) == tuple(int(x) for x in octr[:3]), what + ": ray tallies against the oracle"
        assert int(got["tallies of the render"][3]) == cfg["width"] * cfg["height"] * M, what + ": paths"
    return routes


@pytest.mark.parametrize("chunk", CHUNKS, ids=[f"steps {a}-{b - 1}" for a, b in CHUNKS])
def test_walked_context_equals_fresh_and_oracle(api, oracle_mod, chunk):
    """the context starts at the configuration before the chunk's first step, with every product made once (so that there is state of
    every kind to go wrong), and is led through the chunk's steps: set_config, the three resets, products()"""
    cfgs = RC.configs()
    first, end = chunk
    r = RC.renderer(api, cfgs[first - 1])
    _, routes = RC.products(api, r, cfgs[first - 1])
    for i in range(first, end):
        r.set_config(**RC.WALK[i][1])
        r.reset_accumulation(); r.reset_temporal(); r.reset_baked()
        routes = _check_step(api, oracle_mod, r, i, cfgs[i], routes)
    r.close()


def test_the_first_configuration_against_the_oracle(api, oracle_mod):
    """step 0, which no set_config precedes: the fresh context alone"""
    cfg = RC.configs()[0]
    r = RC.renderer(api, cfg)
    _check_step(api, oracle_mod, r, 0, cfg, None)
    r.close()


# ------------------------------------------------------------------------------------ 2. nothing survives a change of the pixel set
def _live(api, r, one_rank):
    """state of every kind on the context, no reset: 3 samples, mean albedo, a denoised frame, two temporal frames, a baked view"""
    r.render(0, M)
    r.render_guides(0)
    r.accumulate_albedo(0, M)
    r.render_baked(0, M, follow=2, unlit=RC.UNLIT)
    if one_rank:
        r.denoise(iterations=2)
        last = r.inv_projection()
        r.frame_temporal(0, last, iterations=2); r.frame_temporal(1, last, iterations=2)
        assert r.read_temporal()[0][..., 3].max() == 2
        r.render_guides(0); r.accumulate_albedo(0, M)       # (the frames made guides of their own samples)
        r.denoise(iterations=2)
    assert r.read_frame()[0].any() and r.read_moments().any() and r.read_albedo().any() and r.read_baked().any()


def _temporal_pair(r):
    last = r.inv_projection()
    a = r.frame_temporal(0, last, iterations=2)
    b = r.frame_temporal(1, last, ident=a[2].copy(), iterations=2)
    return dict(zip(("data 0", "position 0", "id 0", "out 0", "data 1", "position 1", "id 1", "out 1", "history", "moments", "variance"), a + b + r.read_temporal()))


SAME_COUNT = {kind: i for kind, i in RC.same_count_steps().items()}


@pytest.mark.parametrize("kind", ["shape", "rank", "strip"])
def test_a_new_pixel_set_of_the_same_size_drops_the_frame_state(api, kind, tmp_path):
    cfgs = RC.configs()
    i = SAME_COUNT[kind]
    adaptive = dict(flags=RC.FLAG_ADAPTIVE)
    before, after = dict(cfgs[i - 1], **adaptive), dict(cfgs[i], **adaptive)
    assert before["width"] * len(RC.model_rows(before)) == after["width"] * len(RC.model_rows(after))
    r = RC.renderer(api, before)
    _live(api, r, before["world_size"] == 1)
    r.set_config(**RC.WALK[i][1])
    assert r.local_rows().tolist() == RC.model_rows(after)
    acc, pos, idb = r.read_frame()
    _zero(acc, kind + ": accumulation"); _zero(pos, kind + ": position"); _zero(idb, kind + ": id history")
    _zero(r.read_moments(), kind + ": moments")
    _raises_state(api, r.read_temporal, "pt_read_temporal")
    _raises_state(api, lambda: r.write_denoised_image(tmp_path / "stale.png"), "pt_write_denoised_image")
    _raises_state(api, lambda: r.denoise(iterations=2), "pt_denoise")
    _raises_state(api, r.read_albedo, "pt_read_albedo")
    _raises_state(api, lambda: r.denoise_albedo(api.ALBEDO_MEAN, iterations=2), "pt_denoise_albedo")
    _raises_state(api, r.read_baked, "pt_read_baked")
    for read in (r.read_guides, r.read_guide_instances, r.read_guide_albedo, r.read_guide_hops):       # (buffers of another frame's pixels)
        _raises_state(api, read, read.__name__)
    fresh = RC.renderer(api, after)
    for name, a, b in zip(("accumulation", "position", "id"), r.render(0, M), fresh.render(0, M)):
        assert_bit_equal(a, b, f"{kind}: {name} of a plain render")
    assert_bit_equal(r.read_moments(), fresh.read_moments(), kind + ": moments of a plain render")
    assert r.adaptive_mask(0.05).tolist() == fresh.adaptive_mask(0.05).tolist()
    if after["world_size"] == 1:
        _same(_temporal_pair(r), _temporal_pair(fresh), kind + ": two temporal frames")
    r.close(); fresh.close()


# ------------------------------------------------------------------------------------------------------ 3. what must survive does
KEEPS = [dict(max_bounces=5), dict(seed=RC.SEED1), dict(batch_spp=1), dict(pipelines=1), dict(queue_slack=1024), dict(n_sobol=64), dict(enable_nee=0),
         dict(flags=RC.FLAG_ADAPTIVE | RC.FLAG_NO_LDS_SCENE), dict(stack_lds_levels=RC.SPILL_LEVELS), dict(strip_rows=2), dict(width=32, height=24)]


def test_the_frame_state_survives_a_call_that_keeps_the_pixel_set(api):
    cfg = dict(RC.BASE, flags=RC.FLAG_ADAPTIVE)
    r = RC.renderer(api, cfg)
    _live(api, r, True)
    frame, q, hist = r.read_frame(), r.read_moments(), r.read_temporal()
    mask = r.adaptive_mask(0.05)
    for change in KEEPS:
        what = f"after {change}"
        r.render_guides(0); r.accumulate_albedo(0, M); r.render_baked(0, M, follow=2, unlit=RC.UNLIT)
        r.read_albedo(); r.read_baked(); r.denoise(iterations=2)
        guides = r.read_guides()
        r.set_config(**change)
        for name, a, b in zip(("accumulation", "position", "id"), r.read_frame(), frame):
            assert_bit_equal(a, b, f"{what}: {name}")
        assert_bit_equal(r.read_moments(), q, what + ": moments")
        assert r.adaptive_mask(0.05).tolist() == mask.tolist(), what + ": the moments are still valid"
        for name, a, b in zip(("history", "moments", "variance"), r.read_temporal(), hist):
            assert_bit_equal(a, b, f"{what}: temporal {name}")
        _raises_state(api, lambda: r.denoise(iterations=2), what + ": pt_denoise on stale guides")
        for name, a, b in zip(("position", "normal", "model"), r.read_guides(), guides):
            assert_bit_equal(a, b, f"{what}: the stale guides stay readable, {name}")
        _raises_state(api, r.read_albedo, what + ": pt_read_albedo")
        _raises_state(api, r.read_baked, what + ": pt_read_baked")
    r.close()


def test_adaptive_turned_on_over_samples_waits_for_a_reset(api):
    cfg = dict(RC.BASE)
    r = RC.renderer(api, cfg)
    r.render(0, 2)
    r.set_config(flags=RC.FLAG_ADAPTIVE)
    _raises_state(api, lambda: r.render_adaptive(M, 0.05, 0.0, 2, 0), "pt_render_adaptive over samples without moments")
    _raises_state(api, lambda: r.adaptive_mask(0.05), "pt_adaptive_mask")
    r.reset_accumulation()
    fresh = RC.renderer(api, dict(cfg, flags=RC.FLAG_ADAPTIVE))
    for k in range(2):
        assert r.render_adaptive(M, 0.05, 0.0, 2, 0) == fresh.render_adaptive(M, 0.05, 0.0, 2, 0)
        for name, a, b in zip(("accumulation", "position", "id"), r.read_frame(), fresh.read_frame()):
            assert_bit_equal(a, b, f"round {k}: {name}")
        assert_bit_equal(r.read_moments(), fresh.read_moments(), f"round {k}: moments")
    r.close(); fresh.close()


# -------------------------------------------------------------------------------------------- 4. a refused call on a live context
def test_a_refused_call_on_a_live_context_changes_nothing(api, oracle_mod):
    """another device ordinal once the context has used its own: refused before any device is touched"""
    cfg = dict(RC.BASE, stack_lds_levels=0)
    r = RC.renderer(api, cfg, device=0)
    r.render(0, 2)
    frame, rows, info = r.read_frame(), r.local_rows().tolist(), r.scene_info()
    fields = {name: getattr(r.cfg, name) for name, _ in api.Config._fields_}
    with pytest.raises(api.PtError) as e:
        r.set_config(device=1, width=16, height=12, stack_lds_levels=RC.SPILL_LEVELS, flags=RC.FLAG_NO_LDS_SCENE)
    assert e.value.code == ERR_STATE
    assert {name: getattr(r.cfg, name) for name, _ in api.Config._fields_} == fields, "the wrapper's cfg changed"
    assert r.local_rows().tolist() == rows == RC.model_rows(cfg)
    for name, a, b in zip(("accumulation", "position", "id"), r.read_frame(), frame):
        assert_bit_equal(a, b, "after the refusal: " + name)
    acc, pos, idb = r.render(2, 2, ident=frame[2].copy())
    after = r.scene_info()
    assert (after.uploads_full, after.uploads_patched) == (info.uploads_full, info.uploads_patched), "the refused call made the scene non-resident"
    assert r.stats().lds_scene == 1
    fresh = RC.renderer(api, cfg)
    for name, a, b in zip(("accumulation", "position", "id"), (acc, pos, idb), fresh.render(0, 4)):
        assert_bit_equal(a, b, "render(2, 2) after the refusal against a fresh render(0, 4): " + name)
    oacc = _oracle_render(oracle_mod, cfg, n=4)[0]
    assert_bit_equal(acc, oacc, "... and against the oracle")
    r.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------- 5. pools and uploads
def test_the_pools_follow_size_and_pipelines(api, oracle_mod):
    stops = [dict(width=16, height=12, pipelines=3), dict(width=40, height=24, pipelines=1), dict(width=16, height=12, pipelines=3),
             dict(width=40, height=24, pipelines=2, max_bounces=6), dict(width=24, height=32, pipelines=3, max_bounces=3)]
    cfg = dict(RC.BASE, batch_spp=1, **stops[0])
    r = RC.renderer(api, cfg)
    for k, stop in enumerate(stops):
        if k:
            r.set_config(**stop)
            cfg = dict(cfg, **stop)
        fresh = RC.renderer(api, cfg)
        got, want = r.render(0, M), fresh.render(0, M)
        for name, a, b in zip(("accumulation", "position", "id"), got, want):
            assert_bit_equal(a, b, f"stop {k} {stop}: {name}")
        assert_bit_equal(got[0], _oracle_render(oracle_mod, cfg)[0], f"stop {k}: against the oracle")
        fresh.close()
    r.close()


def test_uploads_follow_the_configuration(api):
    """a change of stack_lds_levels or NO_LDS_SCENE uploads the scene again by the patch path; no other change uploads anything"""
    r = RC.renderer(api, RC.BASE)
    r.render(0, 1)
    info = r.scene_info()
    assert (info.uploads_full, info.uploads_patched) == (1, 0)
    full, patched = 1, 0
    for change, again in ((dict(width=40, height=24), 0), (dict(width=24, height=32), 0), (dict(stack_lds_levels=RC.SPILL_LEVELS), 1),
                          (dict(max_bounces=5, seed=RC.SEED1, n_sobol=64, enable_nee=0), 0), (dict(flags=RC.FLAG_NO_LDS_SCENE), 1),
                          (dict(flags=RC.FLAG_NO_LDS_SCENE | RC.FLAG_GENERAL_WALK | RC.FLAG_ADAPTIVE | RC.FLAG_NO_PRIMARY_CULL), 0),
                          (dict(world_size=2, rank=1), 0), (dict(flags=0, stack_lds_levels=0), 1), (dict(batch_spp=1, pipelines=3, queue_slack=0), 0)):
        r.set_config(**change)
        r.reset_accumulation()
        r.render(0, 1)
        patched += again
        info = r.scene_info()
        assert (info.uploads_full, info.uploads_patched) == (full, patched), change
    r.close()


# ------------------------------------------------------------------------------------- the baked view of a room with lightmaps
def test_the_baked_view_of_a_mapped_room_follows_the_configuration(api):
    """products() bakes a room without maps; here tests/baked_common.py's mapped room alone, its maps set once and kept across the calls"""
    W, H = 37, 19
    sc, maps = BC.mapped_room(W, H)
    r = api.Renderer(sc, W, H, max_bounces=3)
    BC.set_maps(r, maps)
    cfg = dict(width=W, height=H, max_bounces=3)
    seen = []
    for change in ({}, dict(width=19, height=37), dict(world_size=2, rank=1, strip_rows=4), dict(strip_rows=2), dict(world_size=1, rank=0, seed=RC.SEED1),
                   dict(flags=RC.FLAG_NO_LDS_SCENE), dict(width=W, height=H, flags=0)):
        if change:
            r.render_baked(0, 1, follow=1)                     # sums of the old configuration, not reset
            r.set_config(**change)
            cfg = dict(cfg, **change)
            _raises_state(api, r.read_baked, "pt_read_baked after pt_set_config")
        got = r.render_baked(0, M, follow=2, unlit=RC.UNLIT)
        fresh = api.Renderer(sc, **cfg)
        BC.set_maps(fresh, maps)
        assert_bit_equal(got, fresh.render_baked(0, M, follow=2, unlit=RC.UNLIT), f"baked view after {change}")
        assert (got[..., 3] == M).all()
        seen.append(got.tobytes())
        fresh.close()
    assert len(set(seen)) >= 5                                 # the configurations do differ in what they show
    r.close()
