"""GPU (-m gpu): probe visibility on the device, bit for bit: pt_bake_probe_depth against the restated fold of the oracle's trace_closest,
pt_probe_grid_lookup's kernel with depth against the host evaluation (which tests/test_probe_depth_host.py holds to the numpy restatement),
the baked view with depth against the definition restated over oracle pieces (probe_depth_common.baked), the leak of scenes.two_rooms through
the library, the C++ driver and the picture in the Cornell box."""
import numpy as np
import pytest

import baked_common as BC
import guides_follow_common as G
import probe_depth_common as PD
import probe_grid_common as PG
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 37, 19             # test_gpu_probe_grid.py's room and size: several waves with a ragged last block
DEPTH = 3
UNLIT = (0.25, 0.5, 0.125)
RANK_ROWS = [4, 5, 6, 7, 12, 13, 14, 15]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- 1. the bake
N_MAX, FAR = 256, 900.0                                                            # FAR is beyond the room's diagonal: no hit is clamped
_CORNELL = {}


def _cornell(api, O):
    """the Cornell box, its oracle, four probes and the oracle's hits of their first N_MAX rays: made once and left unchanged"""
    if not _CORNELL:
        from path_tracer_amd import scenes
        sc = scenes.cornell_box(48, 32)
        r = api.Renderer(sc, 48, 32)
        by_name = {m.name: m.positions.reshape(-1, 3).astype(np.float64) for m in sc.models}
        tall, short = by_name["cb_box_tall"], by_name["cb_box_short"]
        side = np.array([tall[:, 0].max() + 5.0, 0.0, tall[:, 2].mean()])          # 5 units from the tall box's side
        pos = np.array([[0.0, 200.0, 100.0], side, (short.min(0) + short.max(0)) / 2, [900.0, 50.0, 0.0]], F)
        orc = O.Oracle(sc)
        d = np.array([[r.probe_ray(j, s)[0] for s in range(N_MAX)] for j in range(4)], F)
        tc = [orc.trace_closest(np.repeat(pos[j][None], N_MAX, axis=0), d[j]) for j in range(4)]
        _CORNELL.update(scene=sc, oracle=orc, pos=pos, d=d, t=[c["t"] for c in tc], hit=[c["inst"] != PG.MISS for c in tc])
    return _CORNELL


def _want(c, R, n, far=FAR, first=0, sums=None, counts=None):
    """the fold of samples [first, first + n) of the four probes (keys 0..3) from the cached hits"""
    sums = np.zeros((4, R * R, 2), F) if sums is None else sums.copy()
    counts = np.zeros((4, R * R), np.uint32) if counts is None else counts.copy()
    for j in range(4):
        PD.fold(c["d"][j][first:first + n], c["t"][j][first:first + n], c["hit"][j][first:first + n], R, far, sums[j], counts[j])
    return sums, counts


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert_bit_equal(got[0], want[0], what)


@pytest.mark.parametrize("R", [3, 4, 8])
def test_bake_is_the_fold_of_the_oracles_hits(api, oracle_mod, R):
    c = _cornell(api, oracle_mod)
    r = api.Renderer(c["scene"], 48, 32)
    pos = c["pos"]
    for n in (1, 65, 100, 256):
        want = _want(c, R, n)
        got = r.bake_probe_depth(pos, n, R, FAR)
        _same(got, want, f"R {R}, {n} samples")
        assert (got[1].sum(axis=1) == n).all()
    whole = _want(c, R, 256)
    # the probe inside the short box sees its faces near, the one outside mostly misses
    m = PD.means(*whole, FAR)
    assert m[2][whole[1][2] > 0, 0].max() < 200.0 and (m[3, :, 0] == F(FAR)).any()
    # split ranges continue bit for bit: (0, 100) then (100, 156) is (0, 256)
    a = r.bake_probe_depth(pos, 100, R, FAR)
    _same(a, _want(c, R, 100), "the first part")
    b = r.bake_probe_depth(pos, 156, R, FAR, first_sample=100, sums=a[0], counts=a[1])
    _same(b, whole, "(0, 100) then (100, 156)")
    # tables cut inside a probe's samples
    for batch_spp in (1, 7):
        r2 = api.Renderer(c["scene"], 48, 32, batch_spp=batch_spp)
        _same(r2.bake_probe_depth(pos, 256, R, FAR), whole, f"batch_spp {batch_spp}")
        _same(r2.bake_probe_depth(pos, 100, R, FAR), _want(c, R, 100), f"batch_spp {batch_spp}, 100 samples")
    # continuing from arrays that hold something
    rng = np.random.default_rng(90 + R)
    s0 = rng.uniform(0.0, 500.0, (4, R * R, 2)).astype(F); k0 = rng.integers(0, 1000, (4, R * R)).astype(np.uint32)
    _same(r.bake_probe_depth(pos, 65, R, FAR, sums=s0, counts=k0), _want(c, R, 65, sums=s0, counts=k0), "from non-zero arrays")
    # a max_distance smaller than the room: the clamp bites
    near = 150.0
    clamped = r.bake_probe_depth(pos, 100, R, near)
    _same(clamped, _want(c, R, 100, far=near), "max_distance 150")
    assert not np.array_equal(clamped[0], _want(c, R, 100)[0]) and PD.means(*clamped, near)[..., 0].max() <= F(near)


def test_bake_with_a_key_base_a_first_sample_and_an_empty_world(api, oracle_mod):
    c = _cornell(api, oracle_mod)
    r = api.Renderer(c["scene"], 48, 32)
    pos, R = c["pos"], 4
    # a first sample alone: the cached rays; a key base: other streams, traced again
    _same(r.bake_probe_depth(pos, 65, R, FAR, first_sample=35), _want(c, R, 65, first=35), "first_sample 35")
    want = PD.oracle_depth(c["oracle"], r, pos, 70, R, FAR, first_sample=9, key_base=1000)
    got = r.bake_probe_depth(pos, 70, R, FAR, first_sample=9, key_base=1000)
    _same(got, want, "key_base 1000, first_sample 9")
    assert not np.array_equal(got[0], r.bake_probe_depth(pos, 70, R, FAR, first_sample=9)[0])
    shifted = r.bake_probe_depth(pos[1:], 65, R, FAR, key_base=1)
    whole = _want(c, R, 65)
    _same(shifted, (whole[0][1:], whole[1][1:]), "key_base 1 over probes 1..3")
    # the empty world: every ray counts max_distance
    for m in range(len(c["scene"].models)):
        r.set_instances(m, np.zeros((0, 3, 4), F))
    r.rebuild()
    for R in (3, 8):
        got = r.bake_probe_depth(pos, 100, R, 12.5)
        _same(got, PD.oracle_depth(None, r, pos, 100, R, 12.5), f"empty world, R {R}")
        filled = got[1] > 0
        assert (got[1].sum(axis=1) == 100).all() and (PD.means(*got, 12.5)[filled] == np.array([12.5, 156.25], F)).all()


# ---- 2. the lookup on the device
@pytest.mark.parametrize("count", PG.COUNTS)
def test_device_lookup_with_depth_is_the_host_lookup(api, count):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(48, 32), 48, 32)
    nodes = count[0] * count[1] * count[2]
    for bias, invalid, R in ((0.0, 0.0, 4), (0.375, 0.3, 8)):
        g = PG.random_grid(count, 41 + sum(count), invalid=invalid, bias=bias)
        g.set_on(r)
        P, n = PG.query_points(g, 4096 - nodes - 35, 42)                           # 4 096 points: sixteen blocks
        assert P.shape[0] == 4096
        plain = r.probe_grid_lookup(P, n, on_device=True)
        for facing in (False, True):
            for floor in (0.0, 0.05):
                depth = PD.random_depth(g, R, 43 + R, floor, facing, consistent=not facing)
                depth.set_on(r)
                host, dev = r.probe_grid_lookup(P, n), r.probe_grid_lookup(P, n, on_device=True)
                assert_bit_equal(dev[0], host[0], f"{count}, bias {bias}, facing {facing}, floor {floor}")
                assert np.array_equal(dev[1], host[1])
                assert nodes == 1 or not np.array_equal(dev[0], plain[0])            # (one node: visibility scales E and W alike)
        # the table follows its grid: cleared, the plain kernel's bits; set again, the restatement's
        r.set_probe_grid_depth(None)
        again = r.probe_grid_lookup(P, n, on_device=True)
        assert_bit_equal(again[0], plain[0], f"{count}: depth cleared")
        depth.set_on(r)
        assert_bit_equal(r.probe_grid_lookup(P, n, on_device=True)[0], PD.lookup(g, depth, P, n)[0], f"{count}: the restatement")


# ---- 3. the view in section 22's room
_ROOM = {}


def _room(O):
    """the mapped room at W x H, its maps, the grid, a seeded R = 4 depth table, its oracle and the expected samples: made once"""
    if not _ROOM:
        _ROOM["scene"], _ROOM["maps"] = BC.mapped_room(W, H)
        _ROOM["grid"] = PG.room_grid()
        _ROOM["depth"] = PD.random_depth(_ROOM["grid"], 4, 61, 0.0, True)
        _ROOM["oracle"] = O.Oracle(_ROOM["scene"])
        _ROOM["rays"], _ROOM["want"] = {}, {}
    return _ROOM


def _want_view(O, sample, hops, grid=True, depth=True):
    room = _room(O)
    key = (sample, hops, grid, depth)
    if key not in room["want"]:
        if sample not in room["rays"]:
            room["rays"][sample] = G.pinhole_rays(room["oracle"], W, H, sample)
        B, ending = PD.baked(room["oracle"], room["scene"], room["maps"], room["grid"] if grid else None, room["depth"] if depth else None,
                             *room["rays"][sample], hops, UNLIT)
        room["want"][key] = B.reshape(H, W, 3), ending.reshape(H, W)
    return room["want"][key]


def _renderer(api, O, grid=True, depth=True, **kw):
    room = _room(O)
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH, **kw)
    BC.set_maps(r, room["maps"])
    if grid:
        room["grid"].set_on(r)
        if depth:
            room["depth"].set_on(r)
    return r


def _one(r, sample, follow):
    r.reset_baked()
    s = r.render_baked(sample, 1, follow=follow, unlit=UNLIT)
    assert (s[..., 3] == 1).all()
    return s[..., :3]


@pytest.mark.parametrize("follow", [0, 2])
def test_room_with_depth_matches_the_restated_view(api, oracle_mod, follow):
    r = _renderer(api, oracle_mod)
    for sample in (0, 3):
        want, ending = _want_view(oracle_mod, sample, follow)
        assert_bit_equal(_one(r, sample, follow), want, f"sample {sample}, follow {follow}")
    # visibility changed probe-lit pixels and no others
    plain, plain_ending = _want_view(oracle_mod, 3, follow, depth=False)
    lit = np.isin(plain_ending, (PG.PROBE_UNMAPPED, PG.PROBE_BACK))
    assert (want[lit] != plain[lit]).any() and np.array_equal(want[~lit].view(np.uint32), plain[~lit].view(np.uint32))
    assert {PG.PROBE_UNMAPPED, PG.PROBE_BACK, PG.MAPPED_FRONT, PG.LIGHT} <= set(np.unique(ending).tolist())
    # the sums are the fold of the samples, and (0, a) then (a, b) is (0, a + b)
    r.reset_baked()
    total = r.render_baked(0, 4, follow=follow, unlit=UNLIT)
    assert_bit_equal(total, BC.fold([_want_view(oracle_mod, s, follow)[0] for s in range(4)]), "four samples")
    r.reset_baked()
    r.render_baked(0, 1, follow=follow, unlit=UNLIT)
    assert_bit_equal(r.render_baked(1, 3, follow=follow, unlit=UNLIT), total, "(0, 1) then (1, 3)")


def test_room_with_depth_on_a_rank(api, oracle_mod):
    r = _renderer(api, oracle_mod, rank=1, world_size=2, strip_rows=4)
    assert np.array_equal(r.local_rows().astype(np.int64), RANK_ROWS)
    for follow in (0, 2):
        want, _ = _want_view(oracle_mod, 3, follow)
        assert_bit_equal(_one(r, 3, follow), want[RANK_ROWS], f"rank 1 of 2, follow {follow}")


def test_sums_go_stale_on_depth_and_clearing_restores_the_old_views(api, oracle_mod):
    room = _room(oracle_mod)
    never = _renderer(api, oracle_mod, grid=False)
    bare = never.render_baked(0, 3, follow=2, unlit=UNLIT)
    only_grid = _renderer(api, oracle_mod, depth=False).render_baked(0, 3, follow=2, unlit=UNLIT)
    assert_bit_equal(only_grid, BC.fold([_want_view(oracle_mod, s, 2, depth=False)[0] for s in range(3)]), "a grid alone: the view as it was")
    r = _renderer(api, oracle_mod)
    with_depth = r.render_baked(0, 3, follow=2, unlit=UNLIT)
    assert not np.array_equal(with_depth, only_grid)
    # another depth table: sums that went on would hold 3 + 2 samples
    PD.random_depth(room["grid"], 8, 62, 0.05, False).set_on(r)
    with pytest.raises(api.PtError):
        r.read_baked()
    assert (r.render_baked(3, 2, follow=2, unlit=UNLIT)[..., 3] == 2).all()
    assert (r.render_baked(5, 1, follow=2, unlit=UNLIT)[..., 3] == 3).all()       # an unchanged call continues
    # depth cleared: stale again, and exactly the bits of a grid that never had depth
    r.set_probe_grid_depth(None)
    with pytest.raises(api.PtError):
        r.read_baked()
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), only_grid, "after clearing depth")
    room["depth"].set_on(r)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), with_depth, "depth set again")
    # the grid cleared (its depth with it): exactly the bits of a context that never had a grid
    r.set_probe_grid(None, None, None)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), bare, "after clearing the grid")


# ---- 4. the leak, through the library
def test_two_rooms_view_is_darker_with_depth(api, oracle_mod):
    """scenes.two_rooms seen from the dark room (true radiance 0 on every surface in view): bake_probe_grid's 4 x 2 x 2 grid leaks the lit
    room's light through the partition; with depth_res = 8 the view's mean luminance is strictly below.  Both views equal their
    restatements over the library's own baked tables."""
    from path_tracer_amd import scenes
    Wd, Hd, SPP = 48, 32, PD.TWO_ROOMS_SPP
    sc = scenes.two_rooms(Wd, Hd)
    orc = oracle_mod.Oracle(sc)
    origin, cell = PG.cornell_grid(sc, PD.TWO_ROOMS_COUNT)
    far = PD.two_rooms_max_distance(cell)
    o, d = G.pinhole_rays(orc, Wd, Hd, 0)
    views, means = {}, {}
    for res in (0, 8):
        r = api.Renderer(sc, Wd, Hd, max_bounces=PD.TWO_ROOMS_BOUNCES)
        sums, valid = r.bake_probe_grid(origin, cell, PD.TWO_ROOMS_COUNT, SPP, depth_res=res)
        assert valid.all() and r.probe_grid_depth_info()[0] == res
        view = r.render_baked(0, 1)
        assert (view[..., 3] == 1).all()
        grid = PG.Grid(origin, cell, PD.TWO_ROOMS_COUNT, sums * (F(4.0 * np.pi) / F(SPP)), valid)
        depth = None
        if res:
            pos = r.probe_grid_positions(origin, cell, PD.TWO_ROOMS_COUNT).reshape(-1, 3)
            depth = PD.Depth(PD.means(*r.bake_probe_depth(pos, SPP, res, far), far))
        want, ending = PD.baked(orc, sc, {}, grid, depth, o, d, 0)
        assert_bit_equal(view[..., :3], want.reshape(Hd, Wd, 3), f"two_rooms, depth_res {res}")
        assert (ending == PG.PROBE_UNMAPPED).all()                                   # the camera sees the dark room's surfaces alone
        views[res], means[res] = view, float(BC.luminance(view[..., :3].astype(np.float64)).mean())
    print(f"two_rooms from the dark room: mean luminance {means[0]:.6f} without depth, {means[8]:.6f} with (ratio {means[8] / means[0]:.4f}); the truth is 0")
    assert means[0] > 0.0
    assert means[8] < means[0]


# ---- 5. the C++ surface
def test_headless_probe_depth_writes_the_python_routes_picture(api, tmp_path):
    """examples/headless --probe-grid 4 4 4 64 --probe-depth 8 --baked-view 1 out.png runs and writes the picture the Python route gives,
    which is not the picture without depth"""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_post import _read_png
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, BOUNCES, N, SPP = 48, 32, 4, 4, 64
    exe = B.build_host_driver()
    png = tmp_path / "out.png"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES), "--probe-grid", str(N), str(N), str(N),
                          str(SPP), "--probe-depth", "8", "--baked-view", "1", str(png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    for bad in (["--probe-depth", "8"], ["--probe-grid", "4", "4", "4", "64", "--probe-depth", "17", "--baked-view", "1", str(png)]):
        refused = subprocess.run([exe] + bad, capture_output=True, text=True, cwd=ROOT)
        assert refused.returncode == 2 and "--probe-depth" in refused.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    box = r.active_pixels()[1]
    lo, hi = np.asarray(box[:3], F), np.asarray(box[3:], F)
    cell = ((hi - lo) / F(N)).astype(F)
    origin = (lo + F(0.5) * cell).astype(F)
    r.bake_probe_grid(origin, cell, (N, N, N), SPP)
    plain = r.post_rgb8(r.render_baked(0, 1))
    r.bake_probe_grid(origin, cell, (N, N, N), SPP, depth_res=8)
    assert r.probe_grid_depth_info() == (8, 0, 0.0)
    got = _read_png(png)
    assert np.array_equal(got, r.post_rgb8(r.render_baked(0, 1)))
    assert not np.array_equal(got, plain) and len(np.unique(got.reshape(-1, 3), axis=0)) > 50


# ---- 6. the picture means what the probes mean
def test_probe_lit_view_with_depth_agrees_with_the_path_traced_frame(api):
    """tests/test_gpu_probe_grid.py's end-to-end statistic on its 4 x 4 x 4 grid in the Cornell box, with depth: R = 8, FACING on, vis_floor 0.
    The bound is twice probe_depth_common.DEPTH_FIGURE, derived on the CPU from oracle pieces alone as SH9_FIGURE was (the derivation stands
    there); the margin is section 24's, for the same reason.  Figures: profiles/r25_probe_depth.md."""
    from path_tracer_amd import scenes
    Wd, Hd, B, SPP = PG.E2E_W, PG.E2E_H, PG.E2E_BOUNCES, 16
    sc = scenes.cornell_box(Wd, Hd)
    r = api.Renderer(sc, Wd, Hd, max_bounces=B)
    origin, cell = PG.cornell_grid(sc)

    def mean(acc):
        return float(BC.luminance(acc[..., :3] / acc[..., 3:4]).mean())
    _, valid = r.bake_probe_grid(origin, cell, PG.E2E_COUNT, PG.E2E_PROBE_SPP)
    plain = mean(r.render_baked(0, SPP))
    r.bake_probe_grid(origin, cell, PG.E2E_COUNT, PG.E2E_PROBE_SPP, depth_res=PD.E2E_RES, vis_floor=PD.E2E_FLOOR, facing=PD.E2E_FACING)
    assert r.probe_grid_depth_info() == (PD.E2E_RES, 1, 0.0) and 32 <= int(valid.sum()) < 64
    baked = mean(r.render_baked(0, SPP))
    traced = mean(api.Renderer(sc, Wd, Hd, max_bounces=B + 1).render(0, SPP, want_position=False)[0])
    diff, without, bound = abs(baked - traced) / traced, abs(plain - traced) / traced, 2.0 * PD.DEPTH_FIGURE
    print(f"probe-lit view with depth: mean luminance {baked:.5f}, without depth {plain:.5f}, path traced {traced:.5f}; relative difference {diff:.4f} "
          f"(without depth {without:.4f}); CPU figure {PD.DEPTH_FIGURE:.4f}, bound {bound:.4f}")
    assert diff < bound
