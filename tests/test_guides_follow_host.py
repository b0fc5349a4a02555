"""CPU: the followed guides (pt_render_guides_followed, include/pt_api.h) as far as they go without a device.  pt_guide_follow_dir's host
evaluation against the oracle's material_eval (a mirror is draw-free there; glass wherever the oracle's Fresnel coin chose refraction, and
every total internal reflection) and against the numpy restatement of reflect / refract (guides_follow_common); the errors of the new
entry points, all returned before any device call; and the room the GPU tests render: the oracle alone shows that every case it was built
for occurs, and the restated chain's first hop is the oracle's own first-hit position."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
import guides_follow_common as G
from guides_follow_common import F, H, MISS, W

N = 300
IORS = (1.02, 1.5, 2.4)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _kinds_scene():
    """one tiny triangle per material: a mirror, three glasses and the four kinds the chain ends on"""
    from path_tracer_amd.scene_desc import Camera, Dielectric, Emissive, GGX, Lambertian, Model, SceneDesc, Specular
    mats = [Specular.new((0.9, 0.8, 0.7))] + [Dielectric.new((1.0, 1.0, 1.0), ior, None) for ior in IORS] + [
        Lambertian.new((0.5, 0.5, 0.5)), Emissive.new((3.0, 3.0, 3.0)), GGX.new_metal((0.9, 0.6, 0.2), 0.0), GGX.new_dielectric((1.0, 1.0, 1.0), 0.0, 1.5, None)]
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    nrm = np.broadcast_to(np.array([0, 0, 1], F), tri.shape).copy()
    models = [Model.new(tri + F(3 * k), nrm, m, None, f"m{k}") for k, m in enumerate(mats)]
    return SceneDesc.new(models, Camera.new((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), 60.0, 1.0), "kinds"), mats


@pytest.fixture(scope="module")
def kinds(api, oracle_mod):
    sc, mats = _kinds_scene()
    return api.Renderer(sc, 8, 8, max_bounces=2), oracle_mod.Oracle(sc), mats


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum(axis=-1, keepdims=True))).astype(F)


def _pairs(rng, n, grazing=0):
    """unit normals and unit incoming directions that arrive against them (the normal is face-forwarded: dot(n, i) < 0); the last
    `grazing` rows arrive almost along the surface"""
    nrm = _unit(rng.normal(size=(n, 3)))
    inc = _unit(rng.normal(size=(n, 3)))
    flip = (nrm.astype(np.float64) * inc).sum(axis=1) > 0
    inc[flip] = -inc[flip]
    if grazing:
        t = _unit(np.cross(nrm[-grazing:], rng.normal(size=(grazing, 3))))
        eps = np.geomspace(1e-6, 5e-2, grazing)[:, None]
        inc[-grazing:] = _unit(t - eps * nrm[-grazing:])
    assert ((nrm.astype(np.float64) * inc).sum(axis=1) < 0).all()
    return inc, nrm


def test_new_symbols_are_exported(api):
    L = api.lib()
    header = open(f"{ROOT}/include/pt_api.h").read()
    for name in ("pt_render_guides_followed", "pt_read_guide_hops", "pt_accumulate_albedo_followed", "pt_guide_follow_dir"):
        assert name in api.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    assert "typedef struct pt_guide_params" in header
    assert C.sizeof(api.GuideParams) == 16


def test_mirror_direction_is_the_oracles(kinds):
    r, orc, mats = kinds
    inc, nrm = _pairs(np.random.default_rng(1), N, grazing=20)
    front = np.ones(N, np.uint8)
    got = r.guide_follow_dir(0, inc, nrm, front)
    want = np.stack([orc.material_eval(0, inc[i], nrm[i], 1, i, 0)[:3] for i in range(N)])
    assert_bit_equal(got[:, :3], want, "mirror: follow direction vs the oracle's scatter direction")
    assert (got[:, 3] == 1).all()
    wo, followed, _ = G.follow_dir(mats[0].kind, mats[0].ior, inc, nrm, front)
    assert_bit_equal(got[:, :3], wo, "mirror: follow direction vs the restatement")


@pytest.mark.parametrize("mi", [1, 2, 3], ids=[f"ior{i}" for i in IORS])
def test_glass_direction_is_the_restatement_and_the_oracles_refraction(kinds, mi):
    r, orc, mats = kinds
    rng = np.random.default_rng(10 + mi)
    inc, nrm = _pairs(rng, N, grazing=40)
    front = (np.arange(N) % 2).astype(np.uint8)                # back faces: eta = ior, total internal reflection beyond the critical angle
    got = r.guide_follow_dir(mi, inc, nrm, front)
    wo, followed, tir = G.follow_dir(mats[mi].kind, mats[mi].ior, inc, nrm, front)
    assert_bit_equal(got[:, :3], wo, "glass: follow direction vs the restatement")
    assert (got[:, 3] == 1).all() and not np.isnan(got).any()
    assert tir.any() and (~tir & (front == 0)).any() and (~tir & (front == 1)).any()
    assert not tir[front == 1].any()                           # from outside there is always a refracted ray
    refl = G.reflect(inc, nrm)
    covered = 0
    for i in range(N):
        if tir[i]:
            # refraction is impossible: the oracle reflects under ANY stream
            for s in range(4):
                assert_bit_equal(orc.material_eval(mi, inc[i], nrm[i], int(front[i]), i, s)[:3], got[i, :3], f"row {i}: total internal reflection")
            continue
        for s in range(16):                                    # scan the pixel's streams until the oracle's coin chooses refraction
            d = orc.material_eval(mi, inc[i], nrm[i], int(front[i]), i, s)[:3]
            if not np.array_equal(d.view(np.uint32), refl[i].view(np.uint32)):
                assert_bit_equal(d, got[i, :3], f"row {i}: the oracle's refracted direction")
                covered += 1
                break
    assert 2 * covered >= int((~tir).sum()), (covered, int((~tir).sum()))


def test_other_kinds_end_the_chain(api, kinds):
    r, orc, mats = kinds
    inc, nrm = _pairs(np.random.default_rng(5), 32)
    for mi in range(4, 8):
        for front in (0, 1):
            got = r.guide_follow_dir(mi, inc, nrm, np.full(32, front, np.uint8))
            assert not got.any(), (mi, front)
    with pytest.raises(api.PtError) as e:
        r.guide_follow_dir(8, inc, nrm, np.ones(32, np.uint8))
    assert e.value.code == -1


def _codes(api, r):
    """the return codes of the calls that show the guides' and the sums' state, without changing it"""
    L = r.L
    return (L.pt_read_guides(r.ctx, None, None, None), L.pt_read_guide_hops(r.ctx, None), L.pt_read_guide_instances(r.ctx, None),
            L.pt_read_guide_albedo(r.ctx, None), L.pt_read_albedo(r.ctx, None))


def test_errors_come_before_any_device_call_and_change_nothing(api):
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import SceneDesc
    sc = scenes.cornell_mixed(8, 8)
    r = api.Renderer(sc, 8, 8, max_bounces=2)
    L = r.L
    before = _codes(api, r)
    assert before == (-3, -3, -3, -3, -3)                       # no guides, no sums
    P = api.GuideParams
    bad = [None, P(9), P(0xFFFFFFFF), P(1, (1, 0, 0)), P(0, (0, 0, 7)), P(2, (0, 1, 0))]
    for prm in bad:
        ref = None if prm is None else C.byref(prm)
        assert L.pt_render_guides_followed(r.ctx, 0, ref) == -1, prm
        assert L.pt_accumulate_albedo_followed(r.ctx, 0, 1, ref) == -1, prm
        assert _codes(api, r) == before
    for hops in (0, 3, 8):                                       # what pt_accumulate_albedo refuses
        assert L.pt_accumulate_albedo_followed(r.ctx, 0, 0, C.byref(P(hops))) == -1
        assert L.pt_accumulate_albedo_followed(r.ctx, 0xFFFFFFFF, 2, C.byref(P(hops))) == -1
        assert _codes(api, r) == before
    assert L.pt_render_guides_followed(None, 0, C.byref(P(1))) == -1 and L.pt_read_guide_hops(None, None) == -1
    assert L.pt_accumulate_albedo_followed(None, 0, 1, C.byref(P(1))) == -1
    # PT_ERR_STATE as pt_render_guides: no camera
    nocam = api.Renderer(SceneDesc.new(sc.models, None, "no camera"), 8, 8, max_bounces=2)
    for hops in (0, 2):
        assert L.pt_render_guides_followed(nocam.ctx, 0, C.byref(P(hops))) == -3
        assert L.pt_accumulate_albedo_followed(nocam.ctx, 0, 1, C.byref(P(hops))) == -3
        assert "pt_set_camera" in L.pt_last_error(nocam.ctx).decode()
    assert L.pt_render_guides(nocam.ctx, 0) == -3
    assert _codes(api, nocam) == before
    # the unit hook's host evaluation needs no build, only the material
    z = np.zeros((1, 3), F)
    assert L.pt_guide_follow_dir(r.ctx, 0, 0, 1, None, None, None, None) == -1
    with pytest.raises(api.PtError):
        r.guide_follow_dir(-1, z, z, np.zeros(1, np.uint8))


# ---- the room of the GPU tests, on the oracle alone
@pytest.fixture(scope="module")
def room(oracle_mod):
    sc = G.follow_room()
    orc = oracle_mod.Oracle(sc)
    o, d = G.pinhole_rays(orc, W, H, 0)
    return sc, orc, o, d


def test_restated_first_hop_is_the_oracles_position(room):
    """max_hops = 0 of the restated chain (its fma, its miss) is the first-hit position the oracle's integrator returns"""
    sc, orc, o, d = room
    g = G.chains(orc, sc, o, d, 0)
    want = np.stack([orc.integrate(o[p], d[p], p, 0, max_bounces=1)[1] for p in range(W * H)])
    assert_bit_equal(g["position"], want, "position of the first hit")
    assert not g["hops"].any() and (g["model"] == MISS).any()
    assert (g["model"][g["model"] != MISS] >> 28 == 0).all()


@pytest.mark.parametrize("max_hops", [2, 8])
def test_room_shows_every_case(room, max_hops):
    sc, orc, o, d = room
    g = G.chains(orc, sc, o, d, max_hops)
    counts, via_slab = G.case_counts(g, max_hops)
    print(max_hops, counts)
    assert all(v > 0 for v in counts.values()), counts
    # through the pane: the back face's eta undoes the front face's, so the ray leaves (all but) parallel to how it came
    d0, d2 = g["dirs"][via_slab, 0].astype(np.float64), g["dirs"][via_slab, 2].astype(np.float64)
    cos = (d0 * d2).sum(axis=1) / np.sqrt((d0 * d0).sum(axis=1) * (d2 * d2).sum(axis=1))
    assert (cos > 1 - 1e-9).all(), cos.min()
    d1 = g["dirs"][via_slab, 1].astype(np.float64)
    assert (np.abs((d0 * d1).sum(axis=1) / np.sqrt((d0 * d0).sum(axis=1) * (d1 * d1).sum(axis=1))) < 1 - 1e-4).all()   # ... and was bent inside
    # the textured walls are seen in the tinted mirror, and only there through one hop: tint * (wall colour * texel), exactly
    mirror, wall_a, wall_b = (G.ROOM_MODELS.index(k) for k in ("mirror", "wall_a", "wall_b"))
    tex = sc.models[wall_a].material.texture.data
    tint, base = np.asarray(sc.models[mirror].material.colour, F), np.asarray(sc.models[wall_a].material.colour, F)
    for wall, texel in ((wall_a, tex[0, 0]), (wall_b, tex[0, 1])):
        sel = (g["hop_model"][:, 0] == mirror) & (g["hops"] == 1) & ((g["model"] & 0x0FFFFFFF) == wall)
        assert sel.sum() > 10, (wall, int(sel.sum()))
        assert_bit_equal(g["albedo"][sel], np.broadcast_to(tint * (base * texel), (int(sel.sum()), 3)), "albedo product in the mirror")
        assert (g["model"][sel] >> 28 == 1).all()
    if max_hops == 8:
        assert (g["hops"] == 8).any() and ((g["hops"] > 2) & (g["hops"] < 8)).any()
