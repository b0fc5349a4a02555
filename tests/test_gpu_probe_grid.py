"""GPU (-m gpu): the irradiance volume on the device, bit for bit: pt_probe_grid_lookup's kernel against the host evaluation (which
tests/test_probe_grid_host.py holds to the numpy restatement), the baked view with the probe ending against the definition restated over
oracle pieces (probe_grid_common.baked), and pt_probe_backfaces against the oracle's census."""
import numpy as np
import pytest

import baked_common as BC
import guides_follow_common as G
import probe_grid_common as PG
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 37, 19             # test_gpu_baked.py's room and size: several waves with a ragged last block
DEPTH = 3
UNLIT = (0.25, 0.5, 0.125)
RANK_ROWS = [4, 5, 6, 7, 12, 13, 14, 15]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_ROOM = {}


def _room(O):
    """the mapped room at W x H, its maps, the grid, its oracle and the expected samples: made once and left unchanged"""
    if not _ROOM:
        _ROOM["scene"], _ROOM["maps"] = BC.mapped_room(W, H)
        _ROOM["grid"] = PG.room_grid()
        _ROOM["oracle"] = O.Oracle(_ROOM["scene"])
        _ROOM["rays"], _ROOM["want"] = {}, {}
    return _ROOM


def _want(O, sample, hops, grid=True):
    room = _room(O)
    key = (sample, hops, grid)
    if key not in room["want"]:
        if sample not in room["rays"]:
            room["rays"][sample] = G.pinhole_rays(room["oracle"], W, H, sample)
        B, ending = PG.baked(room["oracle"], room["scene"], room["maps"], room["grid"] if grid else None, *room["rays"][sample], hops, UNLIT)
        room["want"][key] = B.reshape(H, W, 3), ending.reshape(H, W)
    return room["want"][key]


def _renderer(api, O, grid=True, **kw):
    room = _room(O)
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH, **kw)
    BC.set_maps(r, room["maps"])
    if grid:
        room["grid"].set_on(r)
    return r


def _one(r, sample, follow):
    """the baked sample of `sample` alone: fresh sums, so S.rgb = 0 + B = B and S.w = 1"""
    r.reset_baked()
    s = r.render_baked(sample, 1, follow=follow, unlit=UNLIT)
    assert (s[..., 3] == 1).all()
    return s[..., :3]


# ---- 1. the lookup on the device
@pytest.mark.parametrize("count", PG.COUNTS)
def test_device_lookup_is_the_host_lookup(api, count):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(48, 32), 48, 32)
    nodes = count[0] * count[1] * count[2]
    for bias, invalid in ((0.0, 0.0), (0.375, 0.3)):
        g = PG.random_grid(count, 41 + sum(count), invalid=invalid, bias=bias)
        g.set_on(r)
        P, n = PG.query_points(g, 4096 - nodes - 35, 42)                           # 4 096 points: sixteen blocks
        assert P.shape[0] == 4096
        host, dev = r.probe_grid_lookup(P, n), r.probe_grid_lookup(P, n, on_device=True)
        assert_bit_equal(dev[0], host[0], f"{count}, bias {bias}")
        assert np.array_equal(dev[1], host[1]) and bool(host[1].any()) == bool(g.valid.any())
        assert nodes == 1 or ((host[0] > 0).any() and (invalid == 0.0 or not g.valid.all()))
    # the table follows the grid: another grid shows at once
    g = PG.random_grid(count, 43, bias=0.125)
    g.set_on(r)
    assert_bit_equal(r.probe_grid_lookup(P, n, on_device=True)[0], PG.lookup(g, P, n)[0], f"{count}: the restatement")


# ---- 2. the view
@pytest.mark.parametrize("follow", [0, 2])
def test_room_with_a_grid_matches_the_restated_view(api, oracle_mod, follow):
    r = _renderer(api, oracle_mod)
    seen = set()
    for sample in (0, 3):
        want, ending = _want(oracle_mod, sample, follow)
        assert_bit_equal(_one(r, sample, follow), want, f"sample {sample}, follow {follow}")
        seen |= set(np.unique(ending).tolist())
        print(sample, follow, {PG.ENDINGS[k]: int((ending == k).sum()) for k in range(8)})
    # every ending occurs: probe-lit unmapped, probe-lit back face, a mapped front face still from its map, a cell whose corners are all
    # invalid falling to unlit, a light, a miss
    needed = {PG.PROBE_UNMAPPED, PG.PROBE_BACK, PG.MAPPED_FRONT, PG.UNLIT_UNMAPPED, PG.LIGHT, PG.MISS_AT_0} | ({PG.MISS_AFTER_HOPS} if follow else set())
    assert needed <= seen, (needed, seen)
    # the grid changed the probe-lit pixels and no others
    bare, _ = _want(oracle_mod, 3, follow, grid=False)
    lit = np.isin(ending, (PG.PROBE_UNMAPPED, PG.PROBE_BACK))
    assert (want[lit] != bare[lit]).any(axis=1).all() and np.array_equal(want[~lit].view(np.uint32), bare[~lit].view(np.uint32))
    # the sums are the fold of the samples, and (0, a) then (a, b) is (0, a + b)
    r.reset_baked()
    total = r.render_baked(0, 4, follow=follow, unlit=UNLIT)
    assert_bit_equal(total, BC.fold([_want(oracle_mod, s, follow)[0] for s in range(4)]), "four samples")
    r.reset_baked()
    r.render_baked(0, 1, follow=follow, unlit=UNLIT)
    assert_bit_equal(r.render_baked(1, 3, follow=follow, unlit=UNLIT), total, "(0, 1) then (1, 3)")
    assert_bit_equal(r.read_baked(), total, "pt_read_baked")


def test_room_with_a_grid_on_a_rank(api, oracle_mod):
    r = _renderer(api, oracle_mod, rank=1, world_size=2, strip_rows=4)
    assert np.array_equal(r.local_rows().astype(np.int64), RANK_ROWS)
    for follow in (0, 2):
        want, ending = _want(oracle_mod, 3, follow)
        assert_bit_equal(_one(r, 3, follow), want[RANK_ROWS], f"rank 1 of 2, follow {follow}")
        assert {PG.PROBE_UNMAPPED, PG.PROBE_BACK, PG.UNLIT_UNMAPPED, PG.MAPPED_FRONT} <= set(np.unique(ending[RANK_ROWS]).tolist())


def test_sums_go_stale_on_the_grid_and_clearing_it_restores_the_old_view(api, oracle_mod):
    room = _room(oracle_mod)
    never = _renderer(api, oracle_mod, grid=False)
    plain = never.render_baked(0, 3, follow=2, unlit=UNLIT)
    assert_bit_equal(plain, BC.fold([_want(oracle_mod, s, 2, grid=False)[0] for s in range(3)]), "no grid: the view as it was")
    r = _renderer(api, oracle_mod)
    with_grid = r.render_baked(0, 3, follow=2, unlit=UNLIT)
    assert not np.array_equal(with_grid, plain)
    # another grid: sums that went on would hold 3 + 2 samples
    g = room["grid"]
    PG.Grid(g.origin, g.cell, g.count, g.sh * F(0.5), g.valid, g.bias).set_on(r)
    with pytest.raises(api.PtError):
        r.read_baked()
    other = r.render_baked(3, 2, follow=2, unlit=UNLIT)
    assert (other[..., 3] == 2).all()
    # an unchanged call continues
    assert (r.render_baked(5, 1, follow=2, unlit=UNLIT)[..., 3] == 3).all()
    # cleared: exactly the bits of a context that never had a grid
    r.set_probe_grid(None, None, None)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), plain, "after clearing the grid")
    g.set_on(r)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), with_grid, "the grid set again")


# ---- 3. a moved instance is lit where it stands now
def test_a_moved_unmapped_model_is_lit_at_its_new_place(api, oracle_mod):
    room = _room(oracle_mod)
    floor = BC.MAPPED_MODELS.index("floor")
    r = _renderer(api, oracle_mod)
    old = _one(r, 3, 0)
    moved_scene, _ = BC.mapped_room(W, H)
    m = moved_scene.models[floor].matrices.copy()
    m[:, 1, 3] += F(1.5)                                                           # the floor rises into other cells of the grid
    m[:, 0, 3] -= F(2.0)
    moved_scene.models[floor].matrices = m
    orc = oracle_mod.Oracle(moved_scene)
    r.set_instances(floor, m)
    r.rebuild()
    r.set_camera(moved_scene.camera)
    assert r.probe_grid_info()[2] == (3, 2, 4)                                     # world-space data: still there
    want, ending = PG.baked(orc, moved_scene, room["maps"], room["grid"], *G.pinhole_rays(orc, W, H, 3), 0, UNLIT)
    got = _one(r, 3, 0)
    assert_bit_equal(got, want.reshape(H, W, 3), "the moved floor")
    assert (ending == PG.PROBE_UNMAPPED).sum() > 100 and not np.array_equal(got, old)


# ---- 4. the census
def _census_probes(sc):
    """64 probes in the Cornell box: 16 well inside the short box, 16 inside the tall one, 16 in the open room above the boxes, 16 outside"""
    rng = np.random.default_rng(51)
    by_name = {m.name: m.positions.reshape(-1, 3).astype(np.float64) for m in sc.models}

    def around(p, spread):
        lo, hi = p.min(0), p.max(0)
        mid, ext = (lo + hi) / 2, (hi - lo)
        return mid + rng.uniform(-0.5, 0.5, (16, 3)) * ext * spread
    room = by_name["cb_main"]
    lo, hi = room.min(0), room.max(0)
    top = np.array([(lo[0] + hi[0]) / 2, lo[1] + 0.85 * (hi[1] - lo[1]), (lo[2] + hi[2]) / 2])
    open_room = top + rng.uniform(-0.5, 0.5, (16, 3)) * (hi - lo) * np.array([0.6, 0.1, 0.6])
    outside = hi + (hi - lo) * rng.uniform(0.2, 1.0, (16, 3))
    return np.concatenate([around(by_name["cb_box_short"], 0.3), around(by_name["cb_box_tall"], 0.3), open_room, outside]).astype(F)


def test_census_is_the_oracles(api, oracle_mod):
    from path_tracer_amd import scenes
    sc = scenes.cornell_box(48, 32)
    r = api.Renderer(sc, 48, 32)
    orc = oracle_mod.Oracle(sc)
    pos = _census_probes(sc)
    n = 128
    want_hits, want_back = PG.census(orc, r, pos, n)
    hits, back = r.probe_backfaces(pos, n)
    assert np.array_equal(hits, want_hits) and np.array_equal(back, want_back)
    # inside a closed box every ray hits a back face; in the room (open at the front) none does and most rays hit; outside most rays miss
    assert (back[:32] == n).all() and (hits[:32] == n).all()
    assert (back[32:48] == 0).all() and (hits[32:48] > n // 2).all()
    assert (hits[48:] < n // 2).all()
    valid = r.probe_validity(pos, n)
    assert not valid[:32].any() and valid[32:48].all()
    # split sample ranges add up to the whole, and a key base shifts the streams
    a = r.probe_backfaces(pos, 50, first_sample=0)
    b = r.probe_backfaces(pos, 78, first_sample=50)
    assert np.array_equal(a[0] + b[0], hits) and np.array_equal(a[1] + b[1], back)
    shifted = r.probe_backfaces(pos[1:], n, key_base=1)
    assert np.array_equal(shifted[0], hits[1:]) and np.array_equal(shifted[1], back[1:])
    # batches of the ray table cut inside a probe's samples: the counts do not care
    r2 = api.Renderer(sc, 48, 32, batch_spp=3)
    again = r2.probe_backfaces(pos, n)
    assert np.array_equal(again[0], hits) and np.array_equal(again[1], back)


# ---- 5. the picture means what the probes mean
def test_probe_lit_view_agrees_with_the_path_traced_frame(api):
    """The Cornell box at 48 x 32 with NO lightmap: bake_probe_grid bakes probe_grid_common.cornell_grid's 4 x 4 x 4 grid (1 024 samples a
    node, max_bounces = B) and the baked view (16 samples, K = 0) is compared with pt_render of the same frame at max_bounces = B + 1 (a
    baked ray starts one bounce later).  The statistic is section 22's, the relative difference of the two frame-mean luminances.  The
    bound is twice probe_grid_common.SH9_FIGURE, the error band-2 probes on this grid make on this scene as derived on the CPU from oracle
    pieces (the derivation and its reasons stand there); the margin covers the path tracer's own seed-to-seed floor, printed beside it.
    The view WITHOUT the grid (every surface R * unlit = 0, only the light left) must miss the same bound, so that a grid that lights
    nothing cannot pass.  Figures: profiles/r24_probe_grid.md."""
    from path_tracer_amd import scenes
    Wd, Hd, B, SPP = PG.E2E_W, PG.E2E_H, PG.E2E_BOUNCES, 16
    sc = scenes.cornell_box(Wd, Hd)
    r = api.Renderer(sc, Wd, Hd, max_bounces=B)
    origin, cell = PG.cornell_grid(sc)

    def mean(acc):
        return float(BC.luminance(acc[..., :3] / acc[..., 3:4]).mean())
    unlit = mean(r.render_baked(0, SPP))
    _, valid = r.bake_probe_grid(origin, cell, PG.E2E_COUNT, PG.E2E_PROBE_SPP)
    assert r.probe_grid_info()[2] == PG.E2E_COUNT and 32 <= int(valid.sum()) < 64          # nodes inside the two boxes are left out
    baked = mean(r.render_baked(0, SPP))

    def traced(seed):
        p = api.Renderer(sc, Wd, Hd, max_bounces=B + 1, seed=seed)
        return mean(p.render(0, SPP, want_position=False)[0])
    a, b = traced(api.DEFAULT_SEED), traced(12345)
    diff, dark, floor, bound = abs(baked - a) / a, abs(unlit - a) / a, abs(b - a) / a, 2.0 * PG.SH9_FIGURE
    print(f"probe-lit view: mean luminance {baked:.5f}, path traced {a:.5f} (seed 2: {b:.5f}), without a grid {unlit:.5f}; relative difference "
          f"{diff:.4f}, noise floor {floor:.4f}, without a grid {dark:.4f}; CPU figure {PG.SH9_FIGURE:.4f}, bound {bound:.4f}")
    assert diff < bound
    assert dark >= bound


# ---- 6. the C++ surface
def test_headless_probe_grid_lights_the_baked_view(api, tmp_path):
    """examples/headless --probe-grid 3 3 3 16 --baked-view 2 view.png, with no lightmap: the picture is the Python route's, and not the
    black frame the same view gives without a grid"""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_post import _read_png
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, BOUNCES, N, SPP = 48, 32, 4, 3, 16
    exe = B.build_host_driver()
    png = tmp_path / "view.png"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES), "--probe-grid", str(N), str(N), str(N),
                          str(SPP), "--baked-view", "2", str(png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    refused = subprocess.run([exe, "--probe-grid", "3", "3", "0", "16", "--baked-view", "2", str(png)], capture_output=True, text=True, cwd=ROOT)
    assert refused.returncode == 2 and "--probe-grid" in refused.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    dark = r.post_rgb8(r.render_baked(0, 2))
    box = r.active_pixels()[1]
    lo, hi = np.asarray(box[:3], F), np.asarray(box[3:], F)
    cell = ((hi - lo) / F(N)).astype(F)
    _, valid = r.bake_probe_grid((lo + F(0.5) * cell).astype(F), cell, (N, N, N), SPP)
    assert valid.any()
    view = r.render_baked(0, 2)
    got = _read_png(png)
    assert np.array_equal(got, r.post_rgb8(view))
    assert not np.array_equal(got, dark) and len(np.unique(got.reshape(-1, 3), axis=0)) > 50
