"""GPU (-m gpu): directional lightmaps, bit for bit unless said.  The fold against the oracle's per-ray radiance times pt_lightmap_ray's
directions folded in numpy; the gradient and the directional lookup on the device against their host evaluations (which
tests/test_lightmap_directional_host.py holds to the numpy restatements); the baked view against the oracle-walked chains composed with the
restatements (lightmap_directional_common.baked_dir); that nothing moves without a gradient or without a normal-mapped material; and one
statistical test that the directional view is closer to the path-traced picture of a normal-mapped wall than the scalar view is."""
import numpy as np
import pytest

import baked_common as BC
import guides_follow_common as G
import lightmap_common as LC
import lightmap_directional_common as DC
import normalmap_common as NM
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 37, 19
DEPTH = 3
UNLIT = (0.25, 0.5, 0.125)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- 1. the fold
FOLD_W, FOLD_H, FOLD_N, FOLD_SPLIT, FOLD_BATCH = 6, 5, 13, 5, 2
_FOLD = {}


def _fold_scene(which):
    return LC.quad_scene(light=True) if which == "quad" else DC.sparse_soup(light=True)


def _fold_expected(api, O, which):
    """(covered texel indices, per-ray radiance by the oracle, per-ray directions by pt_lightmap_ray), once per scene"""
    if which not in _FOLD:
        sc = _fold_scene(which)
        r = api.Renderer(sc, 48, 32, max_bounces=DEPTH)
        prim, _, position, normal = r.lightmap_texels(0, 0, FOLD_W, FOLD_H)          # host: no GPU
        k = np.flatnonzero(prim.reshape(-1) != LC.MISS)
        P, n = position.reshape(-1, 3)[k], normal.reshape(-1, 3)[k]
        o = (P + F(0.25) * n).astype(F)
        orc = O.Oracle(sc)
        key_base = 100
        d = np.array([r.lightmap_ray(key_base + int(t), s, n[i]) for i, t in enumerate(k) for s in range(FOLD_N)], F)
        rad = np.array([orc.integrate(o[i], d[i * FOLD_N + s], key_base + int(t), s, 1, max_bounces=DEPTH)[0]
                        for i, t in enumerate(k) for s in range(FOLD_N)], F)
        _FOLD[which] = (k, rad, d, key_base)
    return _FOLD[which]


@pytest.mark.parametrize("which", ["quad", "soup"])
def test_fold_against_the_oracle(api, oracle_mod, which):
    """6 x 5 texels, 13 samples as passes of 5 + 8 (the unrolled eight, the tail and the continuation) with wavefront batches of 2 samples,
    three to a ray table: a table's end falls inside a texel's samples in the pass of 8 and in the single pass of 13"""
    k, rad, d, key_base = _fold_expected(api, oracle_mod, which)
    table = 3 * FOLD_BATCH * len(k)
    assert len(k) > 5 and table % (FOLD_N - FOLD_SPLIT) != 0 and table < (FOLD_N - FOLD_SPLIT) * len(k) and table % FOLD_N != 0
    assert (which == "quad") == (len(k) == FOLD_W * FOLD_H)
    rng = np.random.default_rng(3)
    start, start_dir = rng.uniform(-1, 1, (FOLD_H, FOLD_W, 3)).astype(F), rng.uniform(-1, 1, (FOLD_H, FOLD_W, 3, 3)).astype(F)
    want_dir = DC.fold_dir(start_dir, k, rad, d, FOLD_N)
    assert np.abs(want_dir.reshape(-1, 9)[k] - start_dir.reshape(-1, 9)[k]).min() > 0
    sc = _fold_scene(which)
    r = api.Renderer(sc, 48, 32, max_bounces=DEPTH, batch_spp=FOLD_BATCH)
    kw = dict(key_base=key_base, bias=0.25)
    sums, dirs, cov = r.bake_lightmap_directional(0, 0, FOLD_W, FOLD_H, FOLD_SPLIT, sums=start.copy(), dir_sums=start_dir.copy(), **kw)
    sums, dirs, cov = r.bake_lightmap_directional(0, 0, FOLD_W, FOLD_H, FOLD_N - FOLD_SPLIT, first_sample=FOLD_SPLIT, sums=sums, dir_sums=dirs, **kw)
    assert_bit_equal(dirs, want_dir, f"{which}: dir_sum of 5 + 8")
    assert_bit_equal(sums, LC.fold(start, k, rad, FOLD_N), f"{which}: rgb_sum against the oracle")
    plain, plain_cov = r.bake_lightmap(0, 0, FOLD_W, FOLD_H, FOLD_N, sums=start.copy(), **kw)
    assert_bit_equal(sums, plain, f"{which}: rgb_sum is pt_bake_lightmap's")
    assert np.array_equal(cov, plain_cov) and np.array_equal(np.flatnonzero(cov.reshape(-1)), k)
    one_s, one_d, one_c = r.bake_lightmap_directional(0, 0, FOLD_W, FOLD_H, FOLD_N, sums=start.copy(), dir_sums=start_dir.copy(), **kw)
    assert_bit_equal(one_d, dirs, f"{which}: one pass of 13")
    assert_bit_equal(one_s, sums, f"{which}: one pass of 13, sums")
    uncut = api.Renderer(sc, 48, 32, max_bounces=DEPTH)
    assert_bit_equal(uncut.bake_lightmap_directional(0, 0, FOLD_W, FOLD_H, FOLD_N, sums=start.copy(), dir_sums=start_dir.copy(), **kw)[1], dirs, f"{which}: uncut")
    assert_bit_equal(dirs.reshape(-1, 9)[cov.reshape(-1) == 0], start_dir.reshape(-1, 9)[cov.reshape(-1) == 0], f"{which}: uncovered texels")


# ---- 2. the gradient and the lookup: the device against the host
def test_device_gradient_is_the_host_gradient(api):
    sc = DC.sparse_soup()
    r = api.Renderer(sc, 48, 32)
    for inst, (w, h) in ((0, (9, 7)), (1, (33, 17))):                           # one block and a ragged third
        dirs = np.random.default_rng(7 + inst).uniform(-3, 3, (h, w, 3, 3)).astype(F)
        host, dev = r.lightmap_gradient(0, inst, dirs, 13), r.lightmap_gradient(0, inst, dirs, 13, on_device=True)
        assert_bit_equal(dev, host, f"instance {inst}")
        cov = r.lightmap_texels(0, inst, w, h)[0] != LC.MISS
        assert 0 < cov.sum() < w * h and not dev[~cov].any() and np.abs(dev[cov]).min() > 0


def test_device_lookup_is_the_host_lookup(api):
    """normalmap_common's hook scene, a textured scene (the lightmap tables read its UV table): bumpy maps, both faces, a leaf with a map and
    no gradient, a normal-mapped model without UVs or a map; then every gradient cleared"""
    sc = NM.hook_scene()
    r = api.Renderer(sc, 48, 32)
    maps, grads = DC.hook_maps(sc)
    DC.set_all(r, maps, grads)
    q = NM.hook_queries(sc, 3000)
    host, dev = r.lightmap_lookup_directional(*q), r.lightmap_lookup_directional(*q, on_device=True)
    assert_bit_equal(dev[0], host[0], "hook scene")
    scalar = r.lightmap_lookup(*q[:4], on_device=True)
    assert np.array_equal(dev[1], host[1]) and np.array_equal(dev[1], scalar[1]) and host[1].any() and not host[1].all()
    assert not np.array_equal(dev[0], scalar[0])
    for key in grads:
        r.set_lightmap_directional(*key, None)
    assert_bit_equal(r.lightmap_lookup_directional(*q, on_device=True)[0], scalar[0], "no gradient left")


def test_device_lookup_with_one_unmapped_triangle_in_front(api):
    """baked_common.offset_scene: an untextured scene whose compact UV table makes a leaf's way to its UVs the all-ones word; no normal map
    anywhere, so delta = 0 and the gradients must not show"""
    sc, maps = BC.offset_scene()
    r = api.Renderer(sc, 48, 32)
    grads = DC.soup_grads(maps)
    del grads[1, 1]
    DC.set_all(r, maps, grads)
    q = BC.offset_queries(sc)
    d = np.random.default_rng(15).normal(size=(len(q[0]), 3)).astype(F)
    host, dev = r.lightmap_lookup_directional(*q, d), r.lightmap_lookup_directional(*q, d, on_device=True)
    want, want_mapped = BC.scene_lookup(sc, maps, *q)
    assert np.array_equal(dev[1], want_mapped) and np.array_equal(host[1], want_mapped)
    assert_bit_equal(host[0], want, "host")
    assert_bit_equal(dev[0], want, "device")


# ---- 3. the view
_ROOM = {}


def _room(api=None, O=None):
    if "scene" not in _ROOM:
        _ROOM["scene"], _ROOM["maps"], _ROOM["grads"] = DC.rippled_room(W, H)
        _ROOM["rays"], _ROOM["want"] = {}, {}
    if O is not None and "oracle" not in _ROOM:
        _ROOM["oracle"] = O.Oracle(DC.plain_desc(_ROOM["scene"]))
        _ROOM["tlas"] = api.Renderer(_ROOM["scene"], W, H).tlas_instances(0)        # inputs of the definition (host)
    return _ROOM


def _want(api, O, sample, hops, directional=True):
    room = _room(api, O)
    key = (sample, hops, directional)
    if key not in room["want"]:
        if sample not in room["rays"]:
            room["rays"][sample] = G.pinhole_rays(room["oracle"], W, H, sample)
        B, ending, last = DC.baked_dir(room["oracle"], room["scene"], room["maps"], room["grads"] if directional else {}, room["tlas"],
                                       *room["rays"][sample], hops, UNLIT)
        room["want"][key] = B.reshape(H, W, 3), ending.reshape(H, W), last.reshape(H, W)
    return room["want"][key]


def _one(r, sample, follow, unlit=UNLIT):
    r.reset_baked()
    s = r.render_baked(sample, 1, follow=follow, unlit=unlit)
    assert (s[..., 3] == 1).all()
    return s[..., :3]


@pytest.mark.parametrize("follow", [0, 2])
def test_rippled_room_matches_the_restated_view(api, oracle_mod, follow):
    room = _room(api, oracle_mod)
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH)
    DC.set_all(r, room["maps"], room["grads"])
    name = BC.MAPPED_MODELS.index
    for sample in (0, 3):
        want, ending, last = _want(api, oracle_mod, sample, follow)
        scalar, _, _ = _want(api, oracle_mod, sample, follow, directional=False)
        got = _one(r, sample, follow)
        assert_bit_equal(got, want, f"sample {sample}, follow {follow}")
        rippled = (last == name(DC.RIPPLED)) & (ending == BC.MAPPED_FRONT)
        flat = (last == name(DC.FLAT)) & (ending == BC.MAPPED_FRONT)
        assert rippled.sum() > 50 and flat.sum() > 5 and ((last == name(DC.FLAT)) & (ending == BC.MAPPED_BACK)).sum() > 5
        differs = (got.view(np.uint32) != scalar.view(np.uint32)).any(axis=2)
        assert differs[rippled].mean() > 0.9, "the rippled wall is shaded by its normal map"
        assert not differs[~rippled].any(), "the flat wall and everything else is the scalar view's"
    r.reset_baked()
    total = r.render_baked(0, 4, follow=follow, unlit=UNLIT)
    assert_bit_equal(total, BC.fold([_want(api, oracle_mod, s, follow)[0] for s in range(4)]), "four samples")


def test_rippled_room_on_a_rank(api, oracle_mod):
    room = _room(api, oracle_mod)
    r = api.Renderer(room["scene"], W, H, max_bounces=DEPTH, rank=1, world_size=2, strip_rows=4)
    DC.set_all(r, room["maps"], room["grads"])
    rows = r.local_rows().astype(np.int64)
    assert np.array_equal(rows, [4, 5, 6, 7, 12, 13, 14, 15])
    for follow in (0, 2):
        want, _, _ = _want(api, oracle_mod, 3, follow)
        assert_bit_equal(_one(r, 3, follow), want[rows], f"rank 1 of 2, follow {follow}")


# ---- 4. nothing moved
def test_without_a_gradient_or_a_normal_map_the_view_is_what_it_was(api):
    room = _room()
    sc, maps, grads = room["scene"], room["maps"], room["grads"]
    never = api.Renderer(sc, W, H, max_bounces=DEPTH)                              # a context that never sets a gradient
    BC.set_maps(never, maps)
    base = never.render_baked(0, 3, follow=2, unlit=UNLIT)
    base_launches = never.last_launches(api.LAUNCHES_HOOK)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    DC.set_all(r, maps, grads)
    with_grad = r.render_baked(0, 3, follow=2, unlit=UNLIT)
    assert not np.array_equal(with_grad, base) and (with_grad[..., 3] == 3).all()
    # staleness: clearing ONE gradient restarts the sums; clearing all of them gives the other context's bits
    key = (BC.MAPPED_MODELS.index(DC.RIPPLED), 0)
    r.set_lightmap_directional(*key, None)
    assert (r.render_baked(3, 1, follow=2, unlit=UNLIT)[..., 3] == 1).all()
    with pytest.raises(api.PtError):
        r.set_lightmap_directional(*key, grads[key][:-1])
    assert (r.render_baked(4, 1, follow=2, unlit=UNLIT)[..., 3] == 2).all()        # a refused call leaves the sums current
    for k in grads:
        r.set_lightmap_directional(*k, None)
    assert_bit_equal(r.render_baked(0, 3, follow=2, unlit=UNLIT), base, "every gradient cleared")
    assert r.last_launches(api.LAUNCHES_HOOK) == base_launches
    # setting one again restarts them too, and the sums continue across calls
    DC.set_all(r, {}, grads)
    r.render_baked(0, 1, follow=2, unlit=UNLIT)
    assert_bit_equal(r.render_baked(1, 2, follow=2, unlit=UNLIT), with_grad, "(0, 1) then (1, 2)")
    # no normal-mapped material: the gradients are there and nothing reads them
    plain = DC.plain_desc(sc)
    a, b = api.Renderer(plain, W, H, max_bounces=DEPTH), api.Renderer(plain, W, H, max_bounces=DEPTH)
    BC.set_maps(a, maps)
    DC.set_all(b, maps, grads)
    for follow in (0, 2):
        assert_bit_equal(_one(b, 1, follow), _one(a, 1, follow), f"no normal map, follow {follow}")


def test_the_grid_takes_the_perturbed_normal(api):
    """the probe ending's DIR variant: an unmapped, normal-mapped surface under a grid whose light depends on the normal.  Against the
    device's own hooks: pt_probe_grid_lookup at the guides' position with pt_shading_normal's n' (K = 0)"""
    room = _room()
    sc, maps, grads = room["scene"], dict(room["maps"]), room["grads"]
    key = (BC.MAPPED_MODELS.index(DC.RIPPLED), 0)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    del maps[key]                                                                   # the rippled wall is now lit by the grid
    DC.set_all(r, maps, {k: g for k, g in grads.items() if k != key})
    sh = np.random.default_rng(27).uniform(-0.5, 1.5, (2, 2, 2, 9, 3)).astype(F)
    r.set_probe_grid((-40.0, -40.0, -40.0), (80.0, 80.0, 80.0), sh)
    got = _one(r, 0, 0)
    r.render_guides(0)
    pos, nrm, model = r.read_guides()
    wall = (model & 0x0FFFFFFF) == key[0]
    assert wall.sum() > 50
    ys, xs = np.nonzero(wall)
    inst = r.read_guide_instances()[wall]
    albedo = r.read_guide_albedo()[wall]
    # n' from the hook needs the hit's primitive and barycentrics: the camera rays again, through the trace hook
    od = [r.primary_ray(int(y) * W + int(x), 0)[:2] for y, x in zip(ys, xs)]
    o, d = np.array([a for a, _ in od], F), np.array([b for _, b in od], F)
    tc = r.trace_closest(o, d)
    assert np.array_equal(tc["inst"], inst)
    n1, front = r.shading_normal(tc["inst"], tc["prim"], tc["u"], tc["v"], d, on_device=True)
    irr, lit = r.probe_grid_lookup(pos[wall][:, :3], n1, on_device=True)
    irr0, _ = r.probe_grid_lookup(pos[wall][:, :3], nrm[wall], on_device=True)
    assert lit.all() and front.all() and not np.array_equal(irr, irr0)
    assert_bit_equal(got[wall], (albedo * irr).astype(F), "the grid under n'")


def _grid_contexts(api, which):
    """(a context with gradients and the grid `which` in force, one with the same maps and grid that never set a gradient): the rippled wall has
    no map in either, so the grid lights it"""
    room = _room()
    sc, maps, grads = room["scene"], dict(room["maps"]), room["grads"]
    key = (BC.MAPPED_MODELS.index(DC.RIPPLED), 0)
    del maps[key]
    rng = np.random.default_rng(35)
    sh = np.random.default_rng(27).uniform(-0.5, 1.5, (2, 2, 2, 9, 3)).astype(F)
    R, reach = 4, float(np.sqrt(3.0) * 80.0)
    m1 = (rng.uniform(0.3, 1.5, (8, R * R)) * reach).astype(F)
    m2 = (m1 * m1 + (rng.uniform(0.0, 0.3, m1.shape) * reach).astype(F) ** 2).astype(F)
    alphas = (0.05, 0.4, 1.0)
    table = rng.uniform(0.0, 2.0, (8, len(alphas), R * R, 4)).astype(F)
    table[..., 3] = 0.0
    out = []
    for with_grads in (True, False):
        r = api.Renderer(sc, W, H, max_bounces=DEPTH)
        DC.set_all(r, maps, {k: g for k, g in grads.items() if k != key} if with_grads else {})
        r.set_probe_grid((-40.0, -40.0, -40.0), (80.0, 80.0, 80.0), sh)
        if which in ("depth", "both"):
            r.set_probe_grid_depth(np.stack([m1, m2], axis=-1), 0.0, True)
        if which in ("radiance", "both"):
            r.set_probe_grid_radiance(table, alphas)
        out.append(r)
    return out[0], out[1], key[0]


@pytest.mark.parametrize("which", ["depth", "radiance", "both"])
def test_the_grid_with_depth_and_radiance_takes_the_perturbed_normal(api, which):
    """the DIR variants of the visibility ending and of both reflection-probe endings.  K = 0: the rippled wall is the colour times the
    device's own grid lookup (with visibility where depth is set) under pt_shading_normal's n'; every other pixel, the GGX metal floor under
    radiance among them (metal keeps its unperturbed normal), has the bits of the context that never set a gradient and so launches the
    parent's kernels.  K = 2: the same split by the chain's final surface"""
    r, base, wall_model = _grid_contexts(api, which)
    got, want = _one(r, 0, 0), _one(base, 0, 0)
    r.render_guides(0)
    pos, nrm, model = r.read_guides()
    wall = (model & 0x0FFFFFFF) == wall_model
    metal = (model & 0x0FFFFFFF) == BC.MAPPED_MODELS.index("floor")
    assert wall.sum() > 50 and metal.sum() > 20
    assert_bit_equal(got[~wall], want[~wall], f"{which}: every pixel off the rippled wall")
    assert not np.array_equal(got[wall], want[wall])
    ys, xs = np.nonzero(wall)
    od = [r.primary_ray(int(y) * W + int(x), 0)[:2] for y, x in zip(ys, xs)]
    o, d = np.array([a for a, _ in od], F), np.array([b for _, b in od], F)
    tc = r.trace_closest(o, d)
    assert np.array_equal(tc["inst"], r.read_guide_instances()[wall])
    n1, front = r.shading_normal(tc["inst"], tc["prim"], tc["u"], tc["v"], d, on_device=True)
    irr, lit = r.probe_grid_lookup(pos[wall][:, :3], n1, on_device=True)
    assert front.all() and lit.any()
    light = np.where(lit[:, None].astype(bool), irr, np.array(UNLIT, F)[None, :]).astype(F)
    assert_bit_equal(got[wall], (r.read_guide_albedo()[wall] * light).astype(F), f"{which}: the grid under n'")
    got2, want2 = _one(r, 0, 2), _one(base, 0, 2)
    r.render_guides(0, follow=2)
    final = r.read_guides()[2]
    wall2 = (final != 0xFFFFFFFF) & ((final & 0x0FFFFFFF) == wall_model)
    assert (wall2 & ((final >> 28) > 0)).any()                                  # the wall seen through a mirror or the glass
    assert_bit_equal(got2[~wall2], want2[~wall2], f"{which}, K = 2: chains that end off the rippled wall")
    assert not np.array_equal(got2[wall2], want2[wall2])


def test_directional_dilation_is_the_scalar_dilation_plane_by_plane(api):
    """dilate_lightmap_directional: each axis plane through pt_lightmap_dilate with a FRESH copy of the coverage (a plane dilated with the
    bytes the plane before it left would find nothing to fill), and the coverage that comes back is the dilated one"""
    sc, model = LC.cornell_atlas_scene()
    r = api.Renderer(sc, 48, 32)
    cov = (LC.coverage(sc.models[model].uvs, 16, 16)[0] != LC.MISS).astype(np.uint8)
    grad = np.random.default_rng(37).uniform(-2, 2, (16, 16, 3, 3)).astype(F)
    for passes in (1, 3):
        got, got_cov = r.dilate_lightmap_directional(grad, cov, passes)
        for a in range(3):
            want, want_cov = LC.dilate(grad[:, :, a, :], cov, passes)
            assert_bit_equal(got[:, :, a, :], want, f"plane {a}, {passes} passes")
            assert np.array_equal(got_cov, want_cov)
        assert (got_cov == 2).sum() > 0 and not np.array_equal(got, grad)
        assert_bit_equal(got[cov == 1], grad[cov == 1], "covered texels keep their gradient")


def test_headless_directional_matches_the_python_route(api, tmp_path):
    """examples/headless --bake-lightmap 16 16 8 2 map.txt --directional --normal-ripples 8 --baked-view 3 view.png: the bake with first
    moments, the gradient, both dilations, the map and the gradient set on the shell, the ripples under the bake's planar UVs, shown"""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_post import _read_png
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, BOUNCES, N = 48, 32, 4, 8
    exe = B.build_host_driver()
    png, txt = tmp_path / "view.png", tmp_path / "map.txt"
    common = [exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES)]
    run = subprocess.run(common + ["--bake-lightmap", "16", "16", "8", "2", str(txt), "--directional", "--normal-ripples", str(N), "--baked-view", "3", str(png)],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    for bad in (["--directional"], ["--bake-lightmap", "16", "16", "8", "2", str(txt), "--directional", "--lightmap-denoise"],
                ["--bake-lightmap", "16", "16", "8", "2", str(txt), "--normal-ripples", str(N)]):
        assert subprocess.run(common + bad, capture_output=True, text=True, cwd=ROOT).returncode == 2, bad
    src = scenes.cornell_models()
    models = [Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"),
                             m.material.normal_mapped(DC.ripple_texture(N)) if m.name == "cb_main" else m.material) for m in src]
    r = api.Renderer(SceneDesc.new(models, scenes.reference_camera(Wd / Hd)), Wd, Hd, max_bounces=BOUNCES)
    p = r.model_vertices(1)[0].reshape(-1, 3)[:, [0, 2]]
    lo, hi = p.min(0), p.max(0)
    r.set_model_uvs(1, ((p - lo) / (hi - lo)).astype(F).reshape(-1, 3, 2))
    r.rebuild()
    sums, dirs, cov = r.bake_lightmap_directional(1, 0, 16, 16, 8, bias=0.25)
    grad, _ = r.dilate_lightmap_directional(r.lightmap_gradient(1, 0, dirs, 8, on_device=True), cov, 2)
    sums, cov2 = r.dilate_lightmap(sums, cov, 2)
    rows = [line.split() for line in txt.read_text().splitlines()]
    assert_bit_equal(np.array([[float.fromhex(x) for x in v[1:]] for v in rows], np.float64).astype(F).reshape(16, 16, 3), sums, "map.txt")
    r.set_lightmap_sums(1, 0, sums, 8)
    scalar = r.post_rgb8(r.render_baked(0, 3))
    r.set_lightmap_directional(1, 0, grad)
    assert r.lightmap_directional_info(1, 0)
    got = _read_png(png)
    assert np.array_equal(got, r.post_rgb8(r.render_baked(0, 3)))
    assert not np.array_equal(got, scalar)                                      # the ripples show


# ---- 5. the picture
PIC_W = PIC_H = 64
PIC_MAP, PIC_BAKE, PIC_SPP, PIC_REF_SPP, PIC_BOUNCES, PIC_RIPPLES = 32, 4096, 16, 1024, 3, 8
PIC_RATIO_BOUND = 0.95          # twice the measured 0.8116 is 1.62, which is not below 1: the cap applies


def _picture_scene():
    """the Cornell box whose right wall (cb_right, two triangles over the unit UV square) carries the ripple map"""
    import dataclasses
    from path_tracer_amd import scenes
    models = scenes.cornell_models()
    wall = [m.name for m in models].index("cb_right")
    models[wall] = dataclasses.replace(models[wall], material=models[wall].material.normal_mapped(DC.ripple_texture(PIC_RIPPLES)), uvs=LC.QUAD_UV.copy())
    from path_tracer_amd.scene_desc import SceneDesc
    return SceneDesc.new(models, scenes.reference_camera(PIC_W / PIC_H), "rippled cornell"), wall


def test_the_directional_view_is_closer_to_the_path_traced_wall(api):
    """A Cornell side wall under the ceiling light, rippled by a normal map; its 32 x 32 map and first moments baked with 4096 samples at
    max_bounces = B (the wall's two triangles cover every texel: nothing to dilate); the baked view (16 samples, K = 0) with and without the gradient against pt_render of the same frame at
    max_bounces = B + 1 and 1024 samples (a baked ray starts one bounce later).  The statistic is the per-pixel RMSE over the wall's pixels.
    The condition is RMSE(directional) < RMSE(scalar); the ratio is bounded at twice its measured value, and the reference's own
    seed-to-seed RMSE on those pixels must stay below a quarter of the directional view's.  Measured on an MI355X (313 wall pixels, mean
    0.0410): RMSE directional 0.013092, scalar 0.016131, ratio 0.8116; reference seed to seed 0.002825, 0.216 of the directional.  (At 512
    and 2048 bake samples the ratio is 0.8598 and 0.8297: the bake's noise is not what limits it.  The light is a small source about 45
    degrees off the wall's normal, where the linear model's gradient, (8/3) M0 w_t, overshoots the true one, M0 w_t / (n.w), about twofold:
    profiles/r29_directional_lightmaps.md.)"""
    sc, wall = _picture_scene()
    r = api.Renderer(sc, PIC_W, PIC_H, max_bounces=PIC_BOUNCES)
    sums, dirs, cov = r.bake_lightmap_directional(wall, 0, PIC_MAP, PIC_MAP, PIC_BAKE, bias=0.25)
    assert cov.all()
    grad = r.lightmap_gradient(wall, 0, dirs, PIC_BAKE, on_device=True)
    r.set_lightmap_sums(wall, 0, sums, PIC_BAKE)
    r.render_guides(0)
    on_wall = (r.read_guides()[2] & 0x0FFFFFFF) == wall
    assert on_wall.sum() > 300

    def view():
        r.reset_baked()
        s = r.render_baked(0, PIC_SPP)
        return (s[..., :3] / s[..., 3:4]).astype(np.float64)[on_wall]
    scalar = view()
    r.set_lightmap_directional(wall, 0, grad)
    directional = view()

    def traced(seed):
        p = api.Renderer(sc, PIC_W, PIC_H, max_bounces=PIC_BOUNCES + 1, seed=seed)
        acc = p.render(0, PIC_REF_SPP, want_position=False)[0]
        return (acc[..., :3] / acc[..., 3:4]).astype(np.float64)[on_wall]
    ref, ref2 = traced(api.DEFAULT_SEED), traced(12345)
    rmse = lambda a, b: float(np.sqrt(((a - b) ** 2).mean()))
    e_dir, e_scalar, e_ref = rmse(directional, ref), rmse(scalar, ref), rmse(ref2, ref)
    print(f"wall pixels {int(on_wall.sum())}, mean {ref.mean():.5f}: RMSE directional {e_dir:.6f}, scalar {e_scalar:.6f}, ratio {e_dir / e_scalar:.4f}; "
          f"reference seed to seed {e_ref:.6f} ({e_ref / e_dir:.3f} of the directional)")
    assert e_ref < 0.25 * e_dir
    assert e_dir < e_scalar
    assert e_dir / e_scalar < PIC_RATIO_BOUND
