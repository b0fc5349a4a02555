"""GPU (-m gpu): every traversal walk at the top of its per-lane stack.  The chain scenes of stack_bound_common, whose designed rays
test_stack_bound_host.py shows to reach the highest level each walk can, under every split of the stack between LDS and the spill area, with the
BVH in LDS and in global memory, in workgroups of 256, 128 and 64 threads: trace hooks and a small frame, bit for bit against the oracle.
No stack is ever sized below its need here: an entry one level too high shows as a wrong answer of THIS launch (Stack8<false>: the neighbour
lane's level 0 or the next workgroup's LDS) or of the launch beside it (Stack8<true>: its spill region), never as a provoked fault."""
import numpy as np
import pytest

import stack_bound_common as S
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES = 16, 12, 2, 4
NAMES = ["blas_chain_left", "blas_chain_mirrored", "blas_chain_right", "tlas_chain", "ident_chain", "both_chains", "lights_chain", "forked"]
IDENT = {"blas_chain_left", "blas_chain_mirrored", "blas_chain_right", "ident_chain", "lights_chain", "forked"}    # every instance an identity: the IDENT kernels
CONFIGS = ["default", "lds1", "lds2", "ldsE-1", "ldsE", "ldsE+1", "global_bvh"]
CASES = [(n, c) for n in NAMES for c in CONFIGS] + [("ident_chain", "general_walk"), ("blas_chain_right", "general_walk"), ("both_chains", "pipes2"),
                                                     ("lights_chain", "pipes2"), ("blas_chain_mirrored", "pipes2"), ("tlas_chain_mirrored", "lds2")]
DEEP_PLATES = 200        # deep_chain(200): stack_entries 162, whose 64-thread workgroups need more than 64 KiB of LDS with every level there
LIMIT_PLATES = 2600      # deep_chain(2600): stack_entries 335, more LDS than a CU has at any workgroup size when every level is kept there


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """name -> the scene, its rays (designed, then 256 seeded random ones) and the oracle's answers, computed once and left alone"""
    cache = {}

    def get(name):
        if name not in cache:
            sc = S.scene(name)
            o = oracle_mod.Oracle(sc)
            do, dd, dt = S.designed(name)
            ro, rd, rt = S.random_for(name)
            O, D, T = np.concatenate([do, ro]), np.concatenate([dd, rd]), np.concatenate([dt, rt])
            assert len(O) <= 1024
            ref = {"scene": sc, "o": O, "d": D, "t": T}
            for which in (0, 1):
                ref[f"closest{which}"] = o.trace_closest(O, D, which=which)
                ref[f"closest_t{which}"] = o.trace_closest(O, D, T, which=which)
                ref[f"any{which}"] = o.trace_any(O, D, T, which=which)
            ref["samples"] = o.render_samples(W, H, SPP, max_bounces=BOUNCES)
            ref["frame"] = o.render(W, H, SPP, max_bounces=BOUNCES)
            if name not in ("blas_chain_right",):      # (the overflow chain is its own light: its frame is camera rays alone)
                assert int(ref["frame"][3][1]) >= 50 and int(ref["frame"][3][2]) >= 50, (name, ref["frame"][3][:3])      # shadow and next-event rays are cast
            cache[name] = ref
        return cache[name]
    return get


def formula(r, desc):
    """HostScene::flatten's stack_entries, evaluated from the dumped trees"""
    return S.Trees(r, desc).bound()


def expected_geometry(lds_scene, blob, entries, levels):
    """derive_scene_view as the interface documents it: min(entries, levels or 14) levels in LDS, the workgroup halved from 256 towards 64 threads while
    the dynamic LDS (staged BVH + 8 bytes per level and thread) exceeds 64 KiB"""
    stack_lds = min(entries, levels or 14)
    need = lambda t: (blob if lds_scene else 0) + stack_lds * t * 8
    threads = 256
    while threads > 64 and need(threads) > 64 * 1024:
        threads //= 2
    return threads, stack_lds, need(threads)


def check_traces(r, ref, name):
    """both hooks on both TLASes against the oracle; returns the world launches' log rows (launcher, row, axes)"""
    launched = []
    for which in (0, 1):
        g = r.trace_closest(ref["o"], ref["d"], which=which)
        if which == 0:
            launched += [l for l in r.last_launches(1) if l[0] == "closest"]
        for k in ("inst", "prim", "t", "u", "v"):
            assert_bit_equal(g[k], ref[f"closest{which}"][k], f"{name} tlas{which} closest.{k}")
        g = r.trace_closest(ref["o"], ref["d"], ref["t"], which=which)
        for k in ("inst", "prim", "t", "u", "v"):
            assert_bit_equal(g[k], ref[f"closest_t{which}"][k], f"{name} tlas{which} closest with t_max .{k}")
        assert np.array_equal(r.trace_any(ref["o"], ref["d"], ref["t"], which=which), ref[f"any{which}"]), f"{name} tlas{which} any"
        if which == 0:
            launched += [l for l in r.last_launches(1) if l[0] == "any"]
    assert [l[0] for l in launched] == ["closest", "any"], launched
    return launched


def check_frame(r, ref, name):
    assert_bit_equal(r.render_samples(0, SPP), ref["samples"], f"{name} per-sample radiance")
    r.reset_stats(); r.reset_accumulation()
    acc, pos, idb = r.render(0, SPP)
    oacc, opos, oid, octr = ref["frame"]
    assert_bit_equal(acc, oacc, f"{name} frame"); assert_bit_equal(pos, opos, f"{name} first-hit position"); assert np.array_equal(idb, oid)
    st = r.stats()
    assert (st.rays_closest, st.rays_any, st.rays_light_closest) == (int(octr[0]), int(octr[1]), int(octr[2]))


@pytest.mark.parametrize("name,config", CASES)
def test_chain_scene_under_a_stack_configuration(api, reference, name, config):
    ref = reference(name)
    sc = ref["scene"]
    probe = api.Renderer(sc, W, H, max_bounces=BOUNCES)
    entries = formula(probe, sc)
    levels = {"default": 0, "lds1": 1, "lds2": 2, "ldsE-1": entries - 1, "ldsE": entries, "ldsE+1": entries + 1, "global_bvh": 0, "general_walk": 0, "pipes2": 2}[config]
    flags = {"global_bvh": api.FLAG_NO_LDS_SCENE, "general_walk": api.FLAG_GENERAL_WALK}.get(config, 0)
    kw = dict(batch_spp=1, pipelines=2) if config == "pipes2" else {}
    r = api.Renderer(sc, W, H, max_bounces=BOUNCES, stack_lds_levels=levels, flags=flags, **kw)
    geo = r.trace_geometry()
    st = r.stats()
    assert st.stack_entries == entries                                  # the library's bound is the formula over ITS dumped trees
    assert bool(st.lds_scene) == (config != "global_bvh" and st.scene_bytes <= 48 * 1024)       # (forked is too large to stage)
    threads, stack_lds, lds_bytes = expected_geometry(bool(st.lds_scene), st.scene_bytes, entries, levels)
    assert (geo["block_threads"], geo["stack_lds"]) == (threads, stack_lds), (geo, lds_bytes)
    assert lds_bytes <= 64 * 1024                                       # (the launches over 64 KiB have a test of their own)
    if (name, config) == ("blas_chain_right", "ldsE"):
        assert threads == 64
    if (name, config) == ("both_chains", "ldsE"):
        assert threads == 128
    if (name, config) == ("tlas_chain", "ldsE"):
        assert threads == 256
    ident = name in IDENT and config != "general_walk"
    launched = check_traces(r, ref, name)
    spill = entries > stack_lds
    for launcher, _, axes in launched:
        assert axes[-3:] == (int(bool(st.lds_scene)), int(spill), int(ident)), (launcher, axes)
    print(f"{name} {config}: stack_entries {entries}, {stack_lds} levels in LDS, {threads} threads, {lds_bytes} B of LDS, spill {spill}, ident {ident}")
    check_frame(r, ref, name)


@pytest.mark.parametrize("threads", ["1", "8"])
def test_forked_builder_depth_is_the_dumped_depth(api, reference, monkeypatch, threads):
    """stack_entries rests on the SAH run's depth_out, the forked builder's spliced subtrees included (PTMI_BUILD_THREADS is read at every build)"""
    monkeypatch.setenv("PTMI_BUILD_THREADS", threads)
    ref = reference("forked")
    r = api.Renderer(ref["scene"], W, H, max_bounces=BOUNCES, stack_lds_levels=2)
    r.trace_geometry()
    assert r.stats().stack_entries == formula(r, ref["scene"])
    check_traces(r, ref, "forked")


def test_moved_instances_rebuild_the_bound(api, oracle_mod):
    """pt_set_instances rebuilds the TLAS: a chain's instances pulled together make a shallower tree, pushed apart again the chain; stack_entries follows"""
    sc = S.scene("tlas_chain")
    r = api.Renderer(sc, W, H, max_bounces=BOUNCES, stack_lds_levels=2)
    r.trace_geometry()
    deep = r.stats().stack_entries
    assert deep == formula(r, sc) == 17
    chain = sc.models[0].matrices.copy()
    near = chain.copy()
    near[:, 0, 3] = np.arange(len(near), dtype=np.float32) * 3.0 + 1.0
    r.set_instances(0, near); r.rebuild(); r.trace_geometry()
    sc.models[0].matrices = near
    shallow = r.stats().stack_entries
    assert shallow == formula(r, sc) and shallow < deep
    do, dd, dt = S.designed("tlas_chain")
    o = oracle_mod.Oracle(sc)
    for k in ("inst", "prim", "t"):
        assert_bit_equal(r.trace_closest(do, dd)[k], o.trace_closest(do, dd)[k], f"pulled together closest.{k}")
    r.set_instances(0, chain); r.rebuild(); r.trace_geometry()
    sc.models[0].matrices = chain
    assert r.stats().stack_entries == formula(r, sc) == 17
    o = oracle_mod.Oracle(sc)
    for k in ("inst", "prim", "t"):
        assert_bit_equal(r.trace_closest(do, dd)[k], o.trace_closest(do, dd)[k], f"chain again closest.{k}")


def inline_scene(api, levels, **kw):
    """inline_limit(levels): a right-hanging chain of Lambertian plates whose stack_entries == levels, at the default split"""
    sc = S.inline_limit(levels)
    r = api.Renderer(sc, W, H, max_bounces=BOUNCES, **kw)
    geo = r.trace_geometry()
    assert r.stats().stack_entries == levels == formula(r, sc)
    return sc, r, geo


def test_inline_shadow_walk_at_its_limit(api, oracle_mod):
    """The Lambertian pass walks its own shadow rays (inline_any) while nothing spills and the staged BVH plus the stacks of 256 threads plus 1 KiB fit 32 KiB.
    The largest stack_entries that still gets the walk is found from the scenes' own blob sizes, not guessed.  There the geometry reports the walk, no shadow ray
    is queued, and the frame, whose shadow rays climb the right-hanging chain, is the oracle's with the oracle's tallies; one level deeper the walk is off, the
    same rays go through the queued k_any launch, and frame and tallies still are."""
    want = {}
    for levels in range(9, 17):
        sc, r, geo = inline_scene(api, levels)
        blob = r.stats().scene_bytes
        want[levels] = levels <= 14 and blob + levels * 256 * 8 + 1024 <= 32 * 1024
        assert geo["shade_traces_shadow"] == want[levels], (levels, blob, geo)
    last = max(l for l, w in want.items() if w)
    assert not want[last + 1]
    for levels in (last, last + 1):
        sc, r, geo = inline_scene(api, levels)
        o = oracle_mod.Oracle(sc)
        oacc, opos, oid, octr = o.render(W, H, SPP, max_bounces=BOUNCES)
        assert int(octr[1]) >= 50, octr                       # the frame really casts shadow rays
        assert_bit_equal(r.render_samples(0, SPP), o.render_samples(W, H, SPP, max_bounces=BOUNCES), f"inline limit {levels} per-sample radiance")
        r.reset_stats(); r.reset_accumulation()
        acc, pos, idb = r.render(0, SPP)
        assert_bit_equal(acc, oacc, f"inline limit {levels} frame")
        st = r.stats()
        assert (st.rays_closest, st.rays_any, st.rays_light_closest) == (int(octr[0]), int(octr[1]), int(octr[2]))
        queued = [l for l in r.last_launches(0) if l[0] == "any"]
        assert bool(queued) == (levels != last), (levels, queued)       # with the walk inline (and no GGX surface) no shadow launch is left
        do, dd, dt = S.designed(f"inline_limit_{levels}")
        assert np.array_equal(r.trace_any(do, dd, dt), o.trace_any(do, dd, dt))


@pytest.fixture(scope="module")
def deep(api, oracle_mod):
    sc = S.deep_chain(DEEP_PLATES)
    do, dd, dt = S.designed(f"deep_chain_{DEEP_PLATES}")
    ro, rd, rt = S.random_for("deep")
    return sc, oracle_mod.Oracle(sc), np.concatenate([do, ro]), np.concatenate([dd, rd]), np.concatenate([dt, rt])


def deep_renderer(api, sc):
    r = api.Renderer(sc, W, H, max_bounces=BOUNCES, stack_lds_levels=255)
    geo = r.trace_geometry()
    entries = r.stats().stack_entries
    assert entries == formula(r, sc) and geo["stack_lds"] == entries and geo["block_threads"] == 64
    lds = r.stats().scene_bytes + entries * 64 * 8
    assert 64 * 1024 < lds <= 160 * 1024, lds
    return r


def test_more_than_64k_of_lds_one_launch(api, deep):
    """a workgroup of 64 threads with its whole 162-level stack in LDS: more than 64 KiB of dynamic LDS, which the library accepts up to the CU's 160 KiB.
    ONE closest-hit launch: the oracle's answers, or an error code, never stale buffers"""
    sc, o, O, D, T = deep
    r = deep_renderer(api, sc)
    g = r.trace_closest(O, D)
    c = o.trace_closest(O, D)
    for k in ("inst", "prim", "t", "u", "v"):
        assert_bit_equal(g[k], c[k], f"over 64 KiB closest.{k}")


def test_more_than_64k_of_lds_every_walk(api, deep):
    sc, o, O, D, T = deep
    r = deep_renderer(api, sc)
    for which in (0, 1):
        g, c = r.trace_closest(O, D, T, which=which), o.trace_closest(O, D, T, which=which)
        for k in ("inst", "prim", "t", "u", "v"):
            assert_bit_equal(g[k], c[k], f"over 64 KiB tlas{which} closest.{k}")
        assert np.array_equal(r.trace_any(O, D, T, which=which), o.trace_any(O, D, T, which=which))
    assert_bit_equal(r.render_samples(0, SPP), o.render_samples(W, H, SPP, max_bounces=BOUNCES), "over 64 KiB frame")


def test_more_than_64k_of_lds_under_shadow_and_next_event_rays(api, reference):
    """both_chains with ballast in its light's BLAS: a staged BVH of 46 KB and 42 levels of 64 threads are 68 KB of dynamic LDS, in a scene of Lambertian
    plates: the shading pass's shadow rays and the next-event launches run over 64 KiB as well, not the trace hooks and camera rays alone"""
    ref = reference("both_chains_ballast")
    sc = ref["scene"]
    r = api.Renderer(sc, W, H, max_bounces=BOUNCES, stack_lds_levels=255)
    geo = r.trace_geometry()
    st = r.stats()
    assert st.stack_entries == formula(r, sc) == geo["stack_lds"] and geo["block_threads"] == 64 and st.lds_scene
    assert 64 * 1024 < st.scene_bytes + st.stack_entries * 64 * 8 <= 160 * 1024
    check_traces(r, ref, "both_chains_ballast")
    check_frame(r, ref, "both_chains_ballast")


def test_too_deep_for_lds_is_an_error_and_recovers(api, oracle_mod):
    """every level of a 335-level stack in LDS: 64 threads * 8 bytes * 335 exceed a CU's 160 KiB.  The first trace and the first render return PT_ERR_LIMIT,
    nothing is launched, and the same context is right again once the levels are back at their default"""
    sc = S.deep_chain(LIMIT_PLATES)
    r = api.Renderer(sc, W, H, max_bounces=BOUNCES, stack_lds_levels=100000)
    do, dd, dt = S.designed(f"deep_chain_{LIMIT_PLATES}")
    for call in (lambda: r.trace_closest(do, dd), lambda: r.render(0, 1), lambda: r.trace_any(do, dd, dt)):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == -5 and "too deep for the LDS traversal stack" in str(e.value)
        assert r.last_launches(0) == [] and r.last_launches(1) == []
    r.set_config(stack_lds_levels=0)
    geo = r.trace_geometry()
    entries = r.stats().stack_entries
    assert entries == formula(r, sc) and entries * 64 * 8 > 160 * 1024 and geo["stack_lds"] == 14
    o = oracle_mod.Oracle(sc)
    g, c = r.trace_closest(do, dd), o.trace_closest(do, dd)
    for k in ("inst", "prim", "t", "u", "v"):
        assert_bit_equal(g[k], c[k], f"recovered closest.{k}")
    assert np.array_equal(r.trace_any(do, dd, dt), o.trace_any(do, dd, dt))
    assert_bit_equal(r.render_samples(0, 1), o.render_samples(W, H, 1, max_bounces=BOUNCES), "recovered frame")
