"""GPU (-m gpu): reflection probes on the device, bit for bit: pt_bake_probe_radiance against the restated fold of Oracle.integrate,
k_probe_radiance_prefilter against the host evaluation (which tests/test_probe_radiance_host.py holds to the numpy restatement),
pt_probe_grid_specular's kernels against the host evaluation, the baked view with the metal ending against the definition restated over
oracle pieces (probe_radiance_common.baked), and the C++ driver."""
import numpy as np
import pytest

import baked_common as BC
import guides_follow_common as G
import probe_depth_common as PD
import probe_grid_common as PG
import probe_radiance_common as PR
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 37, 19             # test_gpu_probe_grid.py's room and size: several waves with a ragged last block
DEPTH = 3
UNLIT = (0.25, 0.5, 0.125)
RANK_ROWS = [4, 5, 6, 7, 12, 13, 14, 15]
ALPHAS5 = (0.1, 0.2, 0.4, 0.7, 1.0)
ALPHAS8 = (0.05, 0.1, 0.15, 0.25, 0.4, 0.6, 0.8, 1.0)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- 1. the bake
N = 96
_CORNELL = {}


def _cornell(api, O):
    """the Cornell box, its oracle, three probes (inside the tall box, in the open room, outside) and what the oracle integrates along their
    first N rays: made once and left unchanged (it does not depend on R)"""
    if not _CORNELL:
        from path_tracer_amd import scenes
        sc = scenes.cornell_box(48, 32)
        r = api.Renderer(sc, 48, 32, max_bounces=DEPTH)
        tall = {m.name: m.positions.reshape(-1, 3).astype(np.float64) for m in sc.models}["cb_box_tall"]
        pos = np.array([(tall.min(0) + tall.max(0)) / 2, [0.0, 200.0, 100.0], [900.0, 50.0, 0.0]], F)
        orc = O.Oracle(sc)
        d, L = PR.oracle_rays(orc, r, pos, N, DEPTH)
        _CORNELL.update(scene=sc, oracle=orc, pos=pos, d=d, L=L)
    return _CORNELL


def _want(c, R, n, first=0, sums=None, counts=None):
    return PR.fold_rays(c["d"][:, first:first + n], c["L"][:, first:first + n], R, sums, counts)


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert_bit_equal(got[0], want[0], what)


@pytest.mark.parametrize("R", [2, 3, 8, 16])
def test_bake_is_the_fold_of_the_oracles_radiance(api, oracle_mod, R):
    c = _cornell(api, oracle_mod)
    r = api.Renderer(c["scene"], 48, 32, max_bounces=DEPTH)
    pos = c["pos"]
    whole = _want(c, R, N)
    got = r.bake_probe_radiance(pos, N, R)
    _same(got, whole, f"R {R}, {N} samples")
    assert (got[1].sum(axis=1) == N).all() and (got[0] >= 0).all() and got[0][1].any()
    for n in (1, 65):
        _same(r.bake_probe_radiance(pos, n, R), _want(c, R, n), f"R {R}, {n} samples")
    # split ranges continue bit for bit: (0, 40) then (40, 56) is (0, 96)
    a = r.bake_probe_radiance(pos, 40, R)
    _same(a, _want(c, R, 40), "the first part")
    _same(r.bake_probe_radiance(pos, 56, R, first_sample=40, sums=a[0], counts=a[1]), whole, "(0, 40) then (40, 56)")
    # every cut of the ray table
    for batch_spp in (1, 7, 96):
        r2 = api.Renderer(c["scene"], 48, 32, max_bounces=DEPTH, batch_spp=batch_spp)
        _same(r2.bake_probe_radiance(pos, N, R), whole, f"batch_spp {batch_spp}")
    # continuing from arrays that hold something
    rng = np.random.default_rng(90 + R)
    s0 = rng.uniform(0.0, 50.0, (3, R * R, 3)).astype(F); k0 = rng.integers(0, 1000, (3, R * R)).astype(np.uint32)
    _same(r.bake_probe_radiance(pos, 65, R, sums=s0, counts=k0), _want(c, R, 65, sums=s0, counts=k0), "from non-zero arrays")
    # the same rays give bake_probes its coefficients: the frame and the SH bake are not disturbed
    first = r.bake_probes(pos, N)
    r.bake_probe_radiance(pos, N, R)
    assert_bit_equal(r.bake_probes(pos, N), first, "bake_probes around a radiance bake")


def test_bake_with_a_key_base_and_an_empty_world(api, oracle_mod):
    c = _cornell(api, oracle_mod)
    r = api.Renderer(c["scene"], 48, 32, max_bounces=DEPTH)
    pos, R = c["pos"], 4
    d, L = PR.oracle_rays(c["oracle"], r, pos, 40, DEPTH, first_sample=9, key_base=1000)
    _same(r.bake_probe_radiance(pos, 40, R, first_sample=9, key_base=1000), PR.fold_rays(d, L, R), "key_base 1000, first_sample 9")
    whole = _want(c, R, 65)
    _same(r.bake_probe_radiance(pos[1:], 65, R, key_base=1), (whole[0][1:], whole[1][1:]), "key_base 1 over probes 1..2")
    # the empty world: every ray carries the ambient term
    from path_tracer_amd import scenes
    empty = scenes.cornell_box(48, 32)
    for m in empty.models:
        m.matrices = np.zeros((0, 3, 4), F)
    orc = oracle_mod.Oracle(empty)
    for m in range(len(c["scene"].models)):
        r.set_instances(m, np.zeros((0, 3, 4), F))
    r.rebuild()
    d, L = PR.oracle_rays(orc, r, pos, N, DEPTH)
    assert (L == BC.AMBIENT).all()
    for R in (3, 16):
        got = r.bake_probe_radiance(pos, N, R)
        _same(got, PR.fold_rays(d, L, R), f"empty world, R {R}")
        assert (got[1].sum(axis=1) == N).all()


# ---- 2. the prefilter on the device
@pytest.mark.parametrize("R", [2, 3, 16])
@pytest.mark.parametrize("alphas", [(0.3,), ALPHAS8], ids=["1-level", "8-levels"])
@pytest.mark.parametrize("n", [1, 5])
def test_device_prefilter_is_the_host_prefilter(api, R, alphas, n):
    """R = 2 and 3 run a partly filled wave (4 and 9 lanes of 64), R = 16 four full ones; the grid is n * levels workgroups"""
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(48, 32), 48, 32)
    sums, counts = PR.random_maps(n, R, 200 + R + n, empty=0.3)
    host = r.probe_radiance_prefilter(sums, counts, alphas, on_device=False)
    dev = r.probe_radiance_prefilter(sums, counts, alphas, on_device=True)
    assert_bit_equal(dev, host, f"R {R}, {len(alphas)} levels, {n} probes")
    assert dev.shape == (n, len(alphas), R * R, 4) and (dev[..., 3] == 0).all()
    junk = sums.copy(); junk[counts == 0] = np.nan
    assert_bit_equal(r.probe_radiance_prefilter(junk, counts, alphas, on_device=True), host, "what an empty texel's sums hold")
    assert not r.probe_radiance_prefilter(junk, np.zeros_like(counts), alphas, on_device=True).any()


def test_device_prefilter_of_many_probes(api):
    """more workgroups than the device runs at once: 700 probes x 5 levels at R = 8, the device against the host"""
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(48, 32), 48, 32)
    sums, counts = PR.random_maps(700, 8, 77, empty=0.2)
    assert_bit_equal(r.probe_radiance_prefilter(sums, counts, ALPHAS5, on_device=True), r.probe_radiance_prefilter(sums, counts, ALPHAS5, on_device=False),
                     "700 probes")


# ---- 3. the lookup on the device
@pytest.mark.parametrize("count", PG.COUNTS)
def test_device_specular_lookup_is_the_host_lookup(api, count):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(48, 32), 48, 32)
    nodes = count[0] * count[1] * count[2]
    for bias, invalid, R, alphas in ((0.0, 0.0, 4, (0.35,)), (0.375, 0.3, 16, ALPHAS5)):
        g = PG.random_grid(count, 41 + sum(count), invalid=invalid, bias=bias)
        g.set_on(r)
        P, n, d, a = PR.query(g, 4096 - nodes - 35, 42)                             # 4 096 points: sixteen blocks
        assert P.shape[0] == 4096
        a[:6] = [0.0, alphas[0], alphas[-1], 1.5, np.nan, np.inf]; d[20] = np.nan; d[21] = 0.0
        rad = PR.random_radiance(g, R, alphas, 43 + R)
        for depth in (None, PD.random_depth(g, 4, 44, 0.05, True), PD.random_depth(g, 8, 45, 0.0, False, consistent=False)):
            r.set_probe_grid_depth(None)
            if depth is not None:
                depth.set_on(r)
            rad.set_on(r)
            host, dev = r.probe_grid_specular(P, n, d, a), r.probe_grid_specular(P, n, d, a, on_device=True)
            assert_bit_equal(dev[0], host[0], f"{count}, bias {bias}, depth {depth is not None}")
            assert np.array_equal(dev[1], host[1])
            assert_bit_equal(dev[0], PR.specular(g, depth, rad, P, n, d, a)[0], f"{count}: the restatement")
        # the diffuse lookup's kernels are what they were
        assert_bit_equal(r.probe_grid_lookup(P, n, on_device=True)[0], PD.lookup(g, depth, P, n)[0], f"{count}: the diffuse lookup beside it")
        # the table follows its grid: another table, other bits
        other = PR.random_radiance(g, R, alphas, 99)
        other.set_on(r)
        assert_bit_equal(r.probe_grid_specular(P, n, d, a, on_device=True)[0], PR.specular(g, depth, other, P, n, d, a)[0], f"{count}: another table")


# ---- 4. the view in section 22's room, its panel made of metal
_ROOM = {}
METAL = None


def _room(O):
    """the mapped room at W x H with its panel (ONE mapped model of two quads, one seen from the front and one from the back) made GGX metal
    beside the unmapped metal floor, its maps, the grid, a seeded R = 4 depth table and a seeded R = 8 radiance table, its oracle and the
    expected samples: made once"""
    if not _ROOM:
        from path_tracer_amd.scene_desc import GGX
        sc, maps = BC.mapped_room(W, H)
        sc.models[BC.MAPPED_MODELS.index("panel")].material = GGX.new_metal((0.6, 0.9, 0.5), 0.6)
        _ROOM["scene"], _ROOM["maps"] = sc, maps
        _ROOM["grid"] = PG.room_grid()
        _ROOM["depth"] = PD.random_depth(_ROOM["grid"], 4, 61, 0.0, True)
        _ROOM["rad"] = PR.random_radiance(_ROOM["grid"], 8, ALPHAS5, 63)
        _ROOM["oracle"] = O.Oracle(sc)
        _ROOM["rays"], _ROOM["want"] = {}, {}
    return _ROOM


def _want_view(O, sample, hops, depth=False, rad=True):
    room = _room(O)
    key = (sample, hops, depth, rad)
    if key not in room["want"]:
        if sample not in room["rays"]:
            room["rays"][sample] = G.pinhole_rays(room["oracle"], W, H, sample)
        B, ending, on_metal = PR.baked(room["oracle"], room["scene"], room["maps"], room["grid"], room["depth"] if depth else None,
                                       room["rad"] if rad else None, *room["rays"][sample], hops, UNLIT)
        room["want"][key] = B.reshape(H, W, 3), ending.reshape(H, W), on_metal.reshape(H, W)
    return room["want"][key]


def _renderer(api, O, depth=False, rad=True, **kw):
    room = _room(O)
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH, **kw)
    BC.set_maps(r, room["maps"])
    room["grid"].set_on(r)
    if depth:
        room["depth"].set_on(r)
    if rad:
        room["rad"].set_on(r)
    return r


def _one(r, sample, follow):
    r.reset_baked()
    s = r.render_baked(sample, 1, follow=follow, unlit=UNLIT)
    assert (s[..., 3] == 1).all()
    return s[..., :3]


@pytest.mark.parametrize("follow", [0, 2])
@pytest.mark.parametrize("depth", [False, True], ids=["plain", "vis"])
def test_room_with_radiance_matches_the_restated_view(api, oracle_mod, follow, depth):
    r = _renderer(api, oracle_mod, depth=depth)
    seen, unlit_metal = set(), 0
    for sample in (0, 3):
        want, ending, on_metal = _want_view(oracle_mod, sample, follow, depth=depth)
        assert_bit_equal(_one(r, sample, follow), want, f"sample {sample}, follow {follow}, depth {depth}")
        seen |= set(np.unique(ending).tolist())
        unlit_metal += int((on_metal & np.isin(ending, (PG.UNLIT_UNMAPPED, PG.UNLIT_BACK))).sum())
        print(sample, follow, depth, {name: int((ending == k).sum()) for k, name in PR.ENDINGS.items()}, "unlit on metal so far:", unlit_metal)
    # every ending occurs: the metal one on a front and on a back face, a mapped front face still from its map, a probe-lit unmapped surface,
    # a light, a miss at once (and after a hop when following), and a cell whose corners are all invalid falling to unlit.  (No probe-lit or
    # unlit BACK face is left in this room: its only mapped back face is the panel's, which is metal here and lies inside the lit grid.)
    needed = {PR.METAL_FRONT, PR.METAL_BACK, PG.MAPPED_FRONT, PG.PROBE_UNMAPPED, PG.UNLIT_UNMAPPED, PG.LIGHT, PG.MISS_AT_0} | ({PG.MISS_AFTER_HOPS} if follow else set())
    assert needed <= seen, (sorted(needed), sorted(seen))
    # ... and some unlit pixel lies on GGX metal (the floor beyond the grid's two invalid nodes): where the specular lookup is not lit the
    # ending is the probe ending's, which falls to unlit there
    assert unlit_metal > 0
    # radiance changed the metal pixels and no others
    plain = _want_view(oracle_mod, 3, follow, depth=depth, rad=False)[0]
    metal = np.isin(ending, (PR.METAL_FRONT, PR.METAL_BACK))
    assert (want[metal] != plain[metal]).any() and np.array_equal(want[~metal].view(np.uint32), plain[~metal].view(np.uint32))
    # the sums are the fold of the samples, and (0, a) then (a, b) is (0, a + b)
    r.reset_baked()
    total = r.render_baked(0, 4, follow=follow, unlit=UNLIT)
    assert_bit_equal(total, BC.fold([_want_view(oracle_mod, s, follow, depth=depth)[0] for s in range(4)]), "four samples")
    r.reset_baked()
    r.render_baked(0, 1, follow=follow, unlit=UNLIT)
    assert_bit_equal(r.render_baked(1, 3, follow=follow, unlit=UNLIT), total, "(0, 1) then (1, 3)")


def test_room_with_radiance_on_a_rank(api, oracle_mod):
    r = _renderer(api, oracle_mod, rank=1, world_size=2, strip_rows=4)
    assert np.array_equal(r.local_rows().astype(np.int64), RANK_ROWS)
    for follow in (0, 2):
        want = _want_view(oracle_mod, 3, follow)[0]
        assert_bit_equal(_one(r, 3, follow), want[RANK_ROWS], f"rank 1 of 2, follow {follow}")


def test_sums_go_stale_on_radiance_and_clearing_restores_the_old_views(api, oracle_mod):
    room = _room(oracle_mod)
    only_grid = _renderer(api, oracle_mod, rad=False).render_baked(0, 3, follow=2, unlit=UNLIT)
    assert_bit_equal(only_grid, BC.fold([_want_view(oracle_mod, s, 2, rad=False)[0] for s in range(3)]), "a grid alone: the view as it was")
    with_depth = _renderer(api, oracle_mod, depth=True, rad=False).render_baked(0, 3, follow=2, unlit=UNLIT)
    assert_bit_equal(with_depth, BC.fold([_want_view(oracle_mod, s, 2, depth=True, rad=False)[0] for s in range(3)]), "grid and depth: the view as it was")
    r = _renderer(api, oracle_mod)
    with_rad = r.render_baked(0, 3, follow=2, unlit=UNLIT)
    assert not np.array_equal(with_rad, only_grid)
    # another radiance table: sums that went on would hold 3 + 2 samples
    PR.random_radiance(room["grid"], 4, (0.5,), 64).set_on(r)
    with pytest.raises(api.PtError):
        r.read_baked()
    assert (r.render_baked(3, 2, follow=2, unlit=UNLIT)[..., 3] == 2).all()
    assert (r.render_baked(5, 1, follow=2, unlit=UNLIT)[..., 3] == 3).all()       # an unchanged call continues
    # radiance cleared: stale again, and exactly the bits of a grid that never had radiance
    r.set_probe_grid_radiance(None)
    with pytest.raises(api.PtError):
        r.read_baked()
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), only_grid, "after clearing radiance")
    room["rad"].set_on(r)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), with_rad, "radiance set again")
    # depth under radiance, then radiance cleared: the bits of grid and depth alone
    room["depth"].set_on(r)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), BC.fold([_want_view(oracle_mod, s, 2, depth=True)[0] for s in range(3)]), "depth under radiance")
    r.set_probe_grid_radiance(None)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), with_depth, "radiance cleared under depth")
    # the grid cleared (its radiance with it): exactly the bits of a context that never had a grid
    room["rad"].set_on(r)
    r.set_probe_grid(None, None, None)
    never = api.Renderer(room["scene"], W, H, max_bounces=DEPTH)
    BC.set_maps(never, room["maps"])
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), never.render_baked(0, 3, follow=2, unlit=UNLIT), "after clearing the grid")


# ---- 5. the library's own route and the C++ surface
def test_bake_probe_grid_with_radiance_is_its_parts(api, oracle_mod):
    """bake_probe_grid(radiance_res=8) on the Cornell box with a metal tall box: the table it sets is the device prefilter of its own bake,
    the view is the restated view over that table, and the metal pixels are not the diffuse view's"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import GGX, SceneDesc
    Wd, Hd, SPP, Nn = 48, 32, 64, 4
    sc = SceneDesc.new(scenes.cornell_models(tall_material=GGX.new_metal((0.9, 0.8, 0.6), 0.4)), scenes.reference_camera(Wd / Hd), "metal box")
    orc = oracle_mod.Oracle(sc)
    r = api.Renderer(sc, Wd, Hd, max_bounces=DEPTH)
    origin, cell = PG.cornell_grid(sc, (Nn,) * 3)
    sums, valid = r.bake_probe_grid(origin, cell, (Nn,) * 3, SPP)
    assert r.probe_grid_radiance_info() == (0, ())
    diffuse = r.render_baked(0, 1)
    sums2, valid2 = r.bake_probe_grid(origin, cell, (Nn,) * 3, SPP, radiance_res=8)
    assert_bit_equal(sums2, sums, "the SH bake beside a radiance bake")
    assert np.array_equal(valid, valid2)
    assert r.probe_grid_radiance_info() == (8, tuple(float(F(x)) for x in ALPHAS5))
    view = r.render_baked(0, 1)
    pos = r.probe_grid_positions(origin, cell, (Nn,) * 3).reshape(-1, 3)
    table = r.probe_radiance_prefilter(*r.bake_probe_radiance(pos, SPP, 8), ALPHAS5, on_device=True)
    grid = PG.Grid(origin, cell, (Nn,) * 3, sums * (F(4.0 * np.pi) / F(SPP)), valid)
    o, d = G.pinhole_rays(orc, Wd, Hd, 0)
    want, ending, _ = PR.baked(orc, sc, {}, grid, None, PR.Radiance(table, ALPHAS5), o, d, 0)
    assert_bit_equal(view[..., :3], want.reshape(Hd, Wd, 3), "the view over the baked table")
    metal = (ending == PR.METAL_FRONT).reshape(Hd, Wd)
    assert metal.sum() > 40 and (view[metal][:, :3] != diffuse[metal][:, :3]).any()
    assert np.array_equal(view[~metal].view(np.uint32), diffuse[~metal].view(np.uint32))


def test_headless_probe_radiance_writes_the_python_routes_picture(api, tmp_path):
    """examples/headless --metal-box --probe-grid 4 4 4 64 --probe-radiance 8 --baked-view 1 out.png runs and writes the picture the Python
    route gives, which is not the picture without radiance"""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_post import _read_png
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import GGX, Model, SceneDesc
    Wd, Hd, BOUNCES, Nn, SPP = 48, 32, 4, 4, 64
    exe = B.build_host_driver()
    png = tmp_path / "out.png"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES), "--probe-grid", str(Nn), str(Nn), str(Nn),
                          str(SPP), "--probe-radiance", "8", "--metal-box", "--baked-view", "1", str(png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    for bad in (["--probe-radiance", "8"], ["--probe-grid", "4", "4", "4", "64", "--probe-radiance", "17", "--baked-view", "1", str(png)]):
        refused = subprocess.run([exe] + bad, capture_output=True, text=True, cwd=ROOT)
        assert refused.returncode == 2 and "--probe-radiance" in refused.stderr
    src = scenes.cornell_models(tall_material=GGX.new_metal((0.9, 0.8, 0.6), 0.4))
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    box = r.active_pixels()[1]
    lo, hi = np.asarray(box[:3], F), np.asarray(box[3:], F)
    cell = ((hi - lo) / F(Nn)).astype(F)
    origin = (lo + F(0.5) * cell).astype(F)
    r.bake_probe_grid(origin, cell, (Nn, Nn, Nn), SPP)
    plain = r.post_rgb8(r.render_baked(0, 1))
    r.bake_probe_grid(origin, cell, (Nn, Nn, Nn), SPP, radiance_res=8)
    assert r.probe_grid_radiance_info()[0] == 8
    got = _read_png(png)
    assert np.array_equal(got, r.post_rgb8(r.render_baked(0, 1)))
    assert not np.array_equal(got, plain) and len(np.unique(got.reshape(-1, 3), axis=0)) > 50


# ---- 6. the picture means what the metal means
def test_metal_in_the_baked_view_agrees_with_the_path_traced_frame(api, oracle_mod):
    """cornell_models(tall_material=GGX.new_metal((0.9, 0.8, 0.6), 0.4)) at section 24's frame and 4 x 4 x 4 grid, baked by
    bake_probe_grid(..., radiance_res=8): the mean luminance over the pixels whose chain ends on the metal, baked view against pt_render.
    The bound is twice probe_radiance_common.RADIANCE_FIGURE = 0.1469, derived on the CPU from oracle pieces alone (the derivation and what
    goes into it stand there: the split-sum V = N = R assumption, nearest texels and levels, probes a cell away without parallax, and the G
    term's energy loss, which a path pays and R_H * S does not; per face +11.1 % and -63.0 %, the sums +6.0 %).  The view without radiance
    shades the metal as a diffuse surface and is off by +83 % in that derivation: it is asserted to miss the bound.  Measured on the device:
    profiles/r27_probe_radiance.md."""
    Wd, Hd, B, SPP = PG.E2E_W, PG.E2E_H, PG.E2E_BOUNCES, 256
    sc = PR.e2e_scene()
    orc = oracle_mod.Oracle(sc)
    idx = PR.metal_pixels(orc, sc)[0]
    mask = np.zeros(Wd * Hd, bool); mask[idx] = True
    mask = mask.reshape(Hd, Wd)
    assert mask.sum() == 43
    r = api.Renderer(sc, Wd, Hd, max_bounces=B)
    origin, cell = PG.cornell_grid(sc)

    def mean(acc):
        return float(BC.luminance(acc[..., :3] / acc[..., 3:4])[mask].mean())
    _, valid = r.bake_probe_grid(origin, cell, PG.E2E_COUNT, PG.E2E_PROBE_SPP)
    diffuse = mean(r.render_baked(0, SPP))
    r.bake_probe_grid(origin, cell, PG.E2E_COUNT, PG.E2E_PROBE_SPP, radiance_res=PR.E2E_RES, radiance_alphas=PR.E2E_ALPHAS)
    assert r.probe_grid_radiance_info()[0] == PR.E2E_RES and 32 <= int(valid.sum()) < 64
    baked = mean(r.render_baked(0, SPP))
    traced = mean(api.Renderer(sc, Wd, Hd, max_bounces=B + 1).render(0, SPP, want_position=False)[0])
    diff, without, bound = abs(baked - traced) / traced, abs(diffuse - traced) / traced, 2.0 * PR.RADIANCE_FIGURE
    print(f"metal pixels ({int(mask.sum())}): mean luminance {baked:.5f} with radiance, {diffuse:.5f} without, path traced {traced:.5f}; relative difference "
          f"{diff:.4f} (without radiance {without:.4f}); CPU figure {PR.RADIANCE_FIGURE:.4f} (diffuse {PR.DIFFUSE_FIGURE:.4f}), bound {bound:.4f}")
    assert diff < bound
    assert without > bound                                                        # the diffuse metal misses it
