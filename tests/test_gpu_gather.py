"""GPU (-m gpu): baked rays and the final-gather bake (pt_baked_rays, pt_bake_lightmap_gather, pt_bake_lightmap_adaptive_gather), bit for bit
unless said.  Expected values are tests/gather_common.py's composition of the restatements the tree already has: baked_common.baked over the
oracle's trace_closest for the chain, guides_follow_common.chains for its hop count and first hit, lightmap_common's rays,
lightmap_direct_common's light sample, shadow ray and fold; the baked view itself where the rays must equal it; and one statistical test
that the iterated gather converges to what the path tracer bakes."""
import numpy as np
import pytest

import baked_common as BC
import gather_common as GC
import guides_follow_common as G
import lightmap_common as LC
import lightmap_direct_common as LD
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
UNLIT = GC.UNLIT
KEY_BASE = 5000
BIAS = 0.25
NO_LDS_SCENE = 2


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- the mapped room, its oracle, the seeded rays and what the restatement makes of them: made once and left unchanged
_ROOM = {}


def _room(O):
    if not _ROOM:
        _ROOM["scene"], _ROOM["maps"] = BC.mapped_room()
        _ROOM["oracle"] = O.Oracle(_ROOM["scene"])
        _ROOM["rays"] = GC.room_rays()
        _ROOM["want"] = {}
    return _ROOM


def _want(O, hops):
    room = _room(O)
    if hops not in room["want"]:
        o, d = room["rays"]
        B, ending = BC.baked(room["oracle"], room["scene"], room["maps"], o, d, hops, UNLIT)
        room["want"][hops] = (B, ending) + GC.chain_ends(room["oracle"], room["scene"], o, d, hops)
    return room["want"][hops]


def _room_renderer(api, O, **kw):
    room = _room(O)
    r = api.Renderer(room["scene"], G.W, G.H, **kw)
    BC.set_maps(r, room["maps"])
    return r


# ---- 1. the chain, bit for bit
def test_baked_rays_equal_the_restated_chain(api, oracle_mod):
    r = _room_renderer(api, oracle_mod)
    o, d = _room(oracle_mod)["rays"]
    _, ending, _, _ = _want(oracle_mod, 2)
    counts = {name: int((ending == k).sum()) for k, name in BC.ENDINGS.items()}
    assert all(c >= 8 for c in counts.values()), counts               # the condition, from the oracle's endings alone
    for hops in GC.HOPS:
        B, ending, want_hops, want_id = _want(oracle_mod, hops)
        rgb, got_hops, idb = r.baked_rays(o, d, follow=hops, unlit=UNLIT)
        assert_bit_equal(rgb, B, f"max_hops {hops}: rgb")
        assert np.array_equal(got_hops, want_hops), f"max_hops {hops}: hops"
        assert np.array_equal(idb, want_id), f"max_hops {hops}: id"
        assert got_hops.max() <= hops and (hops == 0 or got_hops.max() >= 1)
    assert (idb == 255).sum() >= 8 and len(np.unique(idb)) > 8
    assert len(r.last_launches(api.LAUNCHES_HOOK)) > 0
    # the device variant: the same bits from rays that never leave the GPU
    import torch
    rgbh, idt = r.baked_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), follow=2, unlit=UNLIT)
    B, _, want_hops, want_id = _want(oracle_mod, 2)
    assert_bit_equal(rgbh[:, :3].cpu().numpy(), B, "device rays: rgb")
    assert np.array_equal(rgbh[:, 3].cpu().numpy(), want_hops.astype(F)) and np.array_equal(idt.cpu().numpy(), want_id)


# ---- 2. the view and the rays are one function
def _axis(api, name):
    """(renderer with the axis' state set, what the ending's axes should be) on a 16 x 12 frame, from the set-ups of the axes' own tests"""
    import lightmap_directional_common as DC
    import probe_depth_common as PD
    import probe_grid_common as PG
    import probe_radiance_common as PR
    W, H = 16, 12
    if name == "gradient":
        sc, maps, grads = DC.rippled_room(W, H)
        r = api.Renderer(sc, W, H)
        DC.set_all(r, maps, grads)
        return r
    sc, maps = BC.mapped_room(W, H)
    r = api.Renderer(sc, W, H)
    BC.set_maps(r, maps)
    if name != "plain":
        grid = PG.room_grid()
        grid.set_on(r)
        if name == "depth":
            PD.random_depth(grid, 4, 61, 0.0, True).set_on(r)
        if name == "radiance":
            PR.random_radiance(grid, 8, (0.1, 0.2, 0.4, 0.7, 1.0), 63).set_on(r)
    return r


_VIEWS = {}


@pytest.mark.parametrize("name", ["plain", "grid", "depth", "radiance", "gradient"])
def test_the_view_is_the_rays_of_its_camera(api, name):
    W, H = 16, 12
    r = _axis(api, name)
    o, d = G.library_rays(r, W, range(H), 0)
    r.reset_baked()
    view = r.render_baked(0, 1, follow=2, unlit=UNLIT)
    assert (view[..., 3] == 1).all()
    rgb, hops, _ = r.baked_rays(o, d, follow=2, unlit=UNLIT)
    assert_bit_equal(rgb.reshape(H, W, 3), view[..., :3], name)
    assert hops.max() >= 1
    # the axes are in force: each room-based view differs from the one it builds on
    _VIEWS[name] = view[..., :3].copy()
    for a, b in (("grid", "plain"), ("depth", "grid"), ("radiance", "grid")):
        if name in (a, b) and a in _VIEWS and b in _VIEWS:
            assert (_VIEWS[a] != _VIEWS[b]).any(), (a, b)
    if name == "gradient":
        import lightmap_directional_common as DC
        sc, maps, grads = DC.rippled_room(W, H)
        flat = api.Renderer(sc, W, H)
        DC.set_all(flat, maps, {})
        assert (flat.baked_rays(o, d, follow=2, unlit=UNLIT)[0] != rgb).any()


# ---- 3. ray counts and cuts
def test_a_rays_bits_do_not_depend_on_the_list_or_the_window(api, oracle_mod):
    r = _room_renderer(api, oracle_mod)
    o, d = _room(oracle_mod)["rays"]
    B, _, want_hops, want_id = _want(oracle_mod, 2)
    for n in (1, 63, 64, 65, 255, 256, 257):
        rgb, hops, idb = r.baked_rays(o[:n], d[:n], follow=2, unlit=UNLIT)
        assert_bit_equal(rgb, B[:n], f"{n} rays")
        assert np.array_equal(hops, want_hops[:n]) and np.array_equal(idb, want_id[:n]), n
    rev = slice(299, None, -1)                                          # the same 300 rays in another order, under three windows
    for window in (0, 64, 100):
        rgb, hops, idb = r.baked_rays(o[:300], d[:300], follow=2, unlit=UNLIT, window_rays=window)
        assert_bit_equal(rgb, B[:300], f"window {window}")
        assert np.array_equal(hops, want_hops[:300]) and np.array_equal(idb, want_id[:300]), window
        rgb, hops, idb = r.baked_rays(o[rev], d[rev], follow=2, unlit=UNLIT, window_rays=window)
        assert_bit_equal(rgb, B[rev], f"window {window}, reversed")
        assert np.array_equal(hops, want_hops[rev]) and np.array_equal(idb, want_id[rev]), window
    assert want_hops[:300].max() == 2 and (want_hops[:64] > 0).any() and (want_hops[64:128] > 0).any()   # chains go on in more than one window
    # the BVH in global memory walks the same chains
    g = _room_renderer(api, oracle_mod, flags=NO_LDS_SCENE)
    assert_bit_equal(g.baked_rays(o, d, follow=2, unlit=UNLIT)[0], B, "global BVH")
    # a list whose every ray misses: the ambient term with no arithmetic, hop 0, id 255
    up = np.tile(np.array([0.0, 1.0, 0.0], F), (130, 1))
    high = np.tile(np.array([0.0, 100.0, 0.0], F), (130, 1)) + o[:130]
    rgb, hops, idb = r.baked_rays(high, up, follow=2, unlit=UNLIT, window_rays=64)
    assert_bit_equal(rgb, np.full((130, 3), BC.AMBIENT, F), "every ray misses")
    assert (hops == 0).all() and (idb == 255).all()
    # an empty world
    for m in range(len(_room(oracle_mod)["scene"].models)):
        r.set_instances(m, np.zeros((0, 3, 4), F))
    r.rebuild()
    rgb, hops, idb = r.baked_rays(o[:257], d[:257], follow=2, unlit=UNLIT)
    assert_bit_equal(rgb, np.full((257, 3), BC.AMBIENT, F), "empty world")
    assert (hops == 0).all() and (idb == 255).all()


# ---- 4. untouched state
def test_baked_rays_leave_the_contexts_products_alone(api, oracle_mod):
    r = _room_renderer(api, oracle_mod, max_bounces=3)
    o, d = _room(oracle_mod)["rays"]
    r.render(0, 2)
    r.render_guides(0, follow=2)
    r.render_baked(0, 2, follow=2, unlit=UNLIT)

    def state():
        return [r.read_accumulation(), *r.read_guides(), r.read_guide_albedo(), r.read_guide_hops(), r.read_baked()]

    before = state()
    paths = r.stats().paths
    rgb = r.baked_rays(o, d, follow=2, unlit=UNLIT)[0]
    assert_bit_equal(rgb, _want(oracle_mod, 2)[0], "the rays")
    after = state()                                     # (a stale product would refuse its read)
    for a, b in zip(before, after):
        assert_bit_equal(a, b, "a product of the context moved")
    assert r.stats().paths == paths
    # ... and the sums continue: the view's (0, 2) then (2, 1) is (0, 3) across the call
    total = r.render_baked(2, 1, follow=2, unlit=UNLIT)
    r.reset_baked()
    assert_bit_equal(total, r.render_baked(0, 3, follow=2, unlit=UNLIT), "the baked sums continue across baked_rays")


# ---- 5. the gather bake, bit for bit
LIT_SIZES = {(0, 0): (24, 16), (1, 0): (24, 16)}
CASES = {"room": (0, 0, 24, 16), "crate": (1, 0, 24, 16), "back": (BC.MAPPED_MODELS.index("back"), 0, 16, 16)}
N = 5
_LIT = {}
_EXPECTED = {}


def _lit(O):
    if not _LIT:
        _LIT["scene"], _LIT["placements"] = BC.lit_room()
        _LIT["oracle"] = O.Oracle(_LIT["scene"])
        _LIT["maps"] = GC.random_maps(LIT_SIZES, 3)
    return _LIT


def _case(O, name):
    """(scene, oracle, maps, model, instance, w, h) of a bake case"""
    model, instance, w, h = CASES[name]
    if name == "back":
        room = _room(O)
        return room["scene"], room["oracle"], room["maps"], model, instance, w, h
    lit = _lit(O)
    return lit["scene"], lit["oracle"], lit["maps"], model, instance, w, h


def _expected(O, name, direct, n=N):
    key = (name, direct, n)
    if key not in _EXPECTED:
        sc, orc, maps, model, instance, w, h = _case(O, name)
        _EXPECTED[key] = GC.gather_samples(O, orc, sc, maps, GC.table_of(sc, model, instance, w, h), n, key_base=KEY_BASE, bias=BIAS, follow=2, unlit=UNLIT,
                                           direct=direct)
    return _EXPECTED[key]


def _renderer(api, O, name, **kw):
    sc, _, maps = _case(O, name)[:3]
    r = api.Renderer(sc, 48, 32, **kw)
    BC.set_maps(r, maps)
    return r


def test_the_cases_mean_something(oracle_mod):
    """asserted from the oracle alone: among the gather rays of the direct == 1 cases a first hit on a lamp (its G zeroed), a mapped front
    face and an unlit ending each occur, and in the mapped room some gather ray ends after at least one hop"""
    seen = {name: _expected(oracle_mod, name, True) for name in CASES}
    assert any(s["zeroed"].any() and (s["B"][s["zeroed"]] != 0).any() for s in seen.values())
    assert any((s["ending"] == BC.MAPPED_FRONT).any() for s in seen.values())
    assert any(np.isin(s["ending"], (BC.MAPPED_BACK, BC.UNMAPPED)).any() for s in seen.values())
    assert (seen["back"]["hops"] >= 1).any() and seen["back"]["zeroed"].any()
    assert (seen["room"]["blocked"] & seen["room"]["cast"]).any() and all((s["D"] > 0).any() for s in seen.values())


@pytest.mark.parametrize("moments", [False, True], ids=["sums", "moments"])
@pytest.mark.parametrize("direct", [False, True], ids=["gather", "direct"])
@pytest.mark.parametrize("name", list(CASES))
def test_gather_bake_against_the_composition(api, oracle_mod, name, direct, moments):
    sc, _, _, model, instance, w, h = _case(oracle_mod, name)
    s = _expected(oracle_mod, name, direct)
    rng = np.random.default_rng(5)
    start = rng.uniform(-1, 1, (h, w, 3)).astype(F); start_sq = rng.uniform(0, 1, (h, w)).astype(F)
    want, want_sq = GC.fold(start, start_sq if moments else None, s, N)
    r = _renderer(api, oracle_mod, name)
    before = r.stats().paths
    got = r.bake_lightmap_gather(model, instance, w, h, N, key_base=KEY_BASE, bias=BIAS, sums=start.copy(), sumsq=start_sq.copy() if moments else None, follow=2,
                                 unlit=UNLIT, direct=direct)
    what = f"{name} direct {direct} moments {moments}"
    cov = got[-1]
    assert np.array_equal(cov, (GC.table_of(sc, model, instance, w, h)[0] != LC.MISS).astype(np.uint8)), what + ": coverage"
    assert_bit_equal(got[0], want, what + ": sums")
    assert_bit_equal(got[0][cov == 0], start[cov == 0], what + ": uncovered texels")
    if moments:
        assert_bit_equal(got[1], want_sq, what + ": sumsq")
    assert r.stats().paths - before == len(s["k"]) * N
    assert len(r.last_launches(api.LAUNCHES_HOOK)) > 0


# ---- 6. continuation and cuts
def test_split_bakes_continue_and_the_batch_cut_does_not_show(api, oracle_mod):
    sc, _, _, model, instance, w, h = _case(oracle_mod, "room")
    s = _expected(oracle_mod, "room", True)
    zero = np.zeros((h, w, 3), F); zero_sq = np.zeros((h, w), F)
    want, want_sq = GC.fold(zero, zero_sq, s, N)
    kw = dict(key_base=KEY_BASE, bias=BIAS, follow=2, unlit=UNLIT, direct=True)
    r = _renderer(api, oracle_mod, "room")
    a, a_sq, _ = r.bake_lightmap_gather(model, instance, w, h, 2, moments=True, **kw)
    b, b_sq, _ = r.bake_lightmap_gather(model, instance, w, h, 3, first_sample=2, sums=a, sumsq=a_sq, **kw)
    assert_bit_equal(b, want, "bake(0, 2) then bake(2, 3): sums")
    assert_bit_equal(b_sq, want_sq, "bake(0, 2) then bake(2, 3): sumsq")
    for batch_spp, flags in ((1, 0), (3, 0), (0, NO_LDS_SCENE)):
        c = _renderer(api, oracle_mod, "room", batch_spp=batch_spp, flags=flags)
        whole, whole_sq, _ = c.bake_lightmap_gather(model, instance, w, h, N, moments=True, **kw)
        assert_bit_equal(whole, want, f"batch_spp {batch_spp} flags {flags}: sums")
        assert_bit_equal(whole_sq, want_sq, f"batch_spp {batch_spp} flags {flags}: sumsq")


# ---- 7. the adaptive contract
def test_adaptive_rounds_hold_every_texel_to_the_gather_bake_at_its_count(api, oracle_mod):
    """two rounds of 2 samples on the room's 24 x 16 map; rel_error 0.2 retires most texels after the first (on the restated samples: 80 of
    352 stay active).  n_active is held to pt_lightmap_adaptive_mask on the state that came in, the texels to the plain gather bake"""
    sc, _, _, model, instance, w, h = _case(oracle_mod, "room")
    crit = dict(rel_error=0.2, abs_floor=0.0, min_samples=2, max_samples=0)
    kw = dict(key_base=KEY_BASE, bias=BIAS, follow=2, unlit=UNLIT, direct=True)
    r = _renderer(api, oracle_mod, "room")
    cov = GC.table_of(sc, model, instance, w, h)[0] != LC.MISS
    sums = sq = counts = None
    actives = []
    for rnd in range(2):
        want_active = int(cov.sum()) if rnd == 0 else int(r.lightmap_adaptive_mask(model, instance, sums, sq, counts, **crit).sum())
        sums, sq, counts, cv, n_active = r.bake_lightmap_adaptive_gather(model, instance, w, h, 2, sums=sums, sumsq=sq, counts=counts, **crit, **kw)
        assert n_active == want_active and np.array_equal(cv, cov.astype(np.uint8)), rnd
        actives.append(n_active)
    assert 0 < actives[1] < actives[0], actives
    assert sorted(np.unique(counts[cov]).tolist()) == [2, 4]
    for n in (2, 4):
        whole, whole_sq, _ = r.bake_lightmap_gather(model, instance, w, h, n, moments=True, **kw)
        at = cov & (counts == n)
        assert_bit_equal(sums[at], whole[at], f"texels with {n} samples: sums")
        assert_bit_equal(sq[at], whole_sq[at], f"texels with {n} samples: sumsq")
    # ... and the plain bake at 4 samples is the composition's (so the contract is held to the oracle, not to the library alone)
    s = _expected(oracle_mod, "room", True, 4)
    want, want_sq = GC.fold(np.zeros((h, w, 3), F), np.zeros((h, w), F), s, 4)
    assert_bit_equal(whole, want, "the plain bake at 4 samples")
    assert_bit_equal(whole_sq, want_sq, "the plain bake at 4 samples: sumsq")


# ---- 8. monotone passes
def test_passes_only_add_light(api, oracle_mod):
    """Every operation from a map's texel to a sample is monotone in the maps (a division by n, the dilation's mean, the lookup's blend with
    weights >= 0, a product with a colour >= 0, one add, the fold's adds), so with the same keys pass k + 1 is >= pass k texel by texel, as
    floats.  The room's atlas puts some texel centres exactly on the box's edges, whose gather rays can leave the room; a black environment
    map makes such a miss 0 instead of the constant ambient, so that pass 0 is the fold of the light samples alone, as with no misses"""
    lit = _lit(oracle_mod)
    sc, orc = lit["scene"], lit["oracle"]
    r = api.Renderer(sc, 48, 32)
    r.set_environment(np.zeros((2, 4, 3), F))
    sizes = [LIT_SIZES[p] for p in lit["placements"]]
    n = 8
    passes = r.bake_lightmaps_gather(lit["placements"], sizes, n, 3, bias=BIAS, follow=0, unlit=(0.0, 0.0, 0.0), direct=True)
    for k in range(2):
        for (lo, cov), (hi, _) in zip(passes[k], passes[k + 1]):
            assert (hi[cov != 0] >= lo[cov != 0]).all(), f"pass {k + 1} below pass {k}"
    room0, room1 = (GC.mean_luminance(*passes[k][0], n) for k in (0, 1))
    assert room1 > room0 > 0
    # pass 0: the light samples alone
    key_base = 0
    for (model, instance), (w, h), (got, cov) in zip(lit["placements"], sizes, passes[0]):
        table = GC.table_of(sc, model, instance, w, h)
        k, o, _, _, smp = LC.bake_rays(oracle_mod, table, n, 0, key_base, BIAS)
        nrm = np.repeat(table[3].reshape(-1, 3)[k], n, 0)
        ls = LD.light_samples(LD.LightTable(orc, sc), np.repeat((k + key_base + w * h).astype(np.uint64), n), smp, o, nrm)
        D = np.where((LD.shadowed(orc, o, ls) | ~ls["cast"])[:, None], F(0.0), ls["ce"]).astype(F)
        want, _ = LD.fold(np.zeros((h, w, 3), F), None, k, D, n)
        assert_bit_equal(got, want, f"pass 0 of placement {(model, instance)}")
        key_base += 2 * w * h


# ---- 9. it converges to the path tracer
# Recorded on the MI355X (profiles/r35_lightmap_gather.md), at CONVERGE_N samples on the 24 x 16 maps: D_PT the relative difference of the
# room map's covered-texel mean luminance between two path-traced direct bakes with disjoint keys, D_G the same between the gather after
# CONVERGE_PASSES passes and the path-traced bake.
CONVERGE_N = 64
CONVERGE_PASSES = 12            # truncation <= 0.7^13 < 1 %
CONVERGE_BOUNCES = 16
D_PT = 0.0229                   # (0.0026 on 48 x 32 maps)
D_G = 0.1345                    # above 5 * D_PT: the bias of the texel resolution and the bilinear look-up; 0.0512 on 48 x 32 maps


def converge_figures(api, size=(24, 16), n=CONVERGE_N):
    """(d_pt, d_g) as defined above, at a map size (the profile also shows the doubled one)"""
    sc, placements = BC.lit_room()
    w, h = size
    r = api.Renderer(sc, 48, 32, max_bounces=CONVERGE_BOUNCES)
    px = w * h
    a, cov = r.bake_lightmap_direct(0, 0, w, h, n, key_base=0, bias=BIAS, light_key_base=px)
    b, _ = r.bake_lightmap_direct(0, 0, w, h, n, key_base=10 * px, bias=BIAS, light_key_base=11 * px)
    passes = r.bake_lightmaps_gather(placements, [size, size], n, CONVERGE_PASSES, key_bases=[20 * px, 22 * px], bias=BIAS, follow=0, unlit=(0.0, 0.0, 0.0), direct=True)
    la, lb, lg = (GC.mean_luminance(m, cov, n) for m in (a, b, passes[-1][0][0]))
    return abs(la - lb) / la, abs(lg - la) / la


def test_iterated_gather_converges_to_the_path_traced_bake(api):
    d_pt, d_g = converge_figures(api)
    print(f"d_pt {d_pt:.5f} d_g {d_g:.5f} (recorded: {D_PT}, {D_G})")
    assert d_g <= 2.0 * max(D_PT, D_G), (d_g, D_PT, D_G)
