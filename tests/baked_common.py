"""Shared by tests/test_baked_host.py and tests/test_gpu_baked.py: the lightmap lookup and the baked sample of include/pt_api.h
(pt_lightmap_lookup, pt_render_baked) restated in numpy, every product, sum and difference ONE np.float32 operation in the order the header
writes them; the chain re-walked over the oracle's trace_closest with the final hit kept; and the scenes the tests render.  Nothing here
calls the library's device code."""
import numpy as np

import guides_follow_common as G
import lightmap_common as LC
from path_tracer_amd import scenes
from path_tracer_amd.scene_desc import EMISSIVE, Camera, Dielectric, Emissive, GGX, Lambertian, Model, SceneDesc, Specular
from textures_common import box, scene_surface_colour, world_instance_models

F = np.float32
MISS = 0xFFFFFFFF
AMBIENT = F(0.006)
# how a chain ended (the table of pt_render_baked)
LIGHT, MAPPED_FRONT, MAPPED_BACK, UNMAPPED, MISS_AT_0, MISS_AFTER_HOPS = range(6)
ENDINGS = {LIGHT: "light", MAPPED_FRONT: "mapped front", MAPPED_BACK: "mapped back", UNMAPPED: "unmapped", MISS_AFTER_HOPS: "miss after a hop"}


# ---------------------------------------------------------------------------------------------------------------------------- the lookup
def lookup(tex, uv3, u, v):
    """THE LOOKUP of include/pt_api.h: tex [h, w, 3]; uv3 [n, 3, 2] the hit triangles' UVs (load-order vertices); u, v [n] -> [n, 3]"""
    tex = np.asarray(tex, F)
    h, w = tex.shape[0], tex.shape[1]
    uv3 = np.asarray(uv3, F); u = np.asarray(u, F); v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore"):
        st = []
        for k in (0, 1):
            a, b, c = uv3[:, 0, k], uv3[:, 1, k], uv3[:, 2, k]
            st.append((a + u * (b - a)) + v * (c - a))
        idx, frac = [], []
        for x, n in ((F(w) * st[0] - F(0.5), w), (F(h) * st[1] - F(0.5), h)):
            top = F(n - 1)
            x = np.where(~(x > F(0.0)), F(0.0), np.where(x > top, top, x)).astype(F)
            x0 = np.trunc(x).astype(np.int64)
            idx.append((x0, np.where(x0 + 1 < n, x0 + 1, x0)))
            frac.append(x - np.trunc(x))
    (x0, x1), (y0, y1) = idx
    xf, yf = frac
    assert xf.dtype == F and yf.dtype == F
    c00, c01, c10, c11 = tex[y0, x0], tex[y1, x0], tex[y0, x1], tex[y1, x1]
    one = F(1.0)
    w00 = ((one - xf) * (one - yf))[:, None]
    w01 = ((one - xf) * yf)[:, None]
    w10 = (xf * (one - yf))[:, None]
    w11 = (xf * yf)[:, None]
    out = ((w00 * c00 + w01 * c01) + w10 * c10) + w11 * c11
    assert out.dtype == F
    return out


def leaf_keys(desc):
    """(model, ordinal) of every world-TLAS leaf in allocation order"""
    return [(i, j) for i, m in enumerate(desc.models) for j in range(m.matrices.shape[0])]


def scene_lookup(desc, maps, instance, prim, u, v):
    """(rgb [n, 3], mapped [n]) of hits on a scene description; maps: {(model, ordinal): [h, w, 3]}"""
    instance = np.asarray(instance, np.int64); prim = np.asarray(prim, np.int64)
    u = np.asarray(u, F); v = np.asarray(v, F)
    keys = leaf_keys(desc)
    out = np.zeros((len(instance), 3), F); mapped = np.zeros(len(instance), np.uint8)
    for leaf in np.unique(instance):
        key = keys[int(leaf)]
        if key not in maps:
            continue
        sel = np.nonzero(instance == leaf)[0]
        out[sel] = lookup(maps[key], desc.models[key[0]].uvs[prim[sel]], u[sel], v[sel])
        mapped[sel] = 1
    return out, mapped


def set_maps(r, maps):
    for (model, ordinal), tex in maps.items():
        r.set_lightmap(model, ordinal, tex)


# ------------------------------------------------------------------------------------------------------------------------------ the chain
def baked(orc, desc, maps, o, d, max_hops, unlit=(0.0, 0.0, 0.0)):
    """the baked sample B [n, 3] of rays (o, d) [n, 3] followed through `desc` (the oracle `orc` holds the same scene) under the constant
    ambient, and how every chain ended [n] (LIGHT .. MISS_AFTER_HOPS): guides_follow_common.chains' walk with the final hit kept"""
    o = np.asarray(o, F).reshape(-1, 3).copy(); d = np.asarray(d, F).reshape(-1, 3).copy()
    n = o.shape[0]
    unlit = np.asarray(unlit, F)
    leaf_model = world_instance_models(desc)
    B = np.zeros((n, 3), F); ending = np.full(n, -1, np.int64)
    live = np.arange(n)
    prod = None
    for h in range(max_hops + 1):
        if live.size == 0:
            break
        tc = orc.trace_closest(o, d)
        hit = tc["inst"] != MISS
        miss = live[~hit]
        B[miss] = AMBIENT if prod is None else prod[~hit] * AMBIENT               # B = E at H = 0, with no arithmetic
        ending[miss] = MISS_AFTER_HOPS if h else MISS_AT_0
        live, o, d = live[hit], o[hit], d[hit]
        if prod is not None:
            prod = prod[hit]
        inst, prim, t = tc["inst"][hit], tc["prim"][hit], tc["t"][hit]
        u, v = tc["u"][hit], tc["v"][hit]
        nrm, front = tc["normal"][hit], tc["front"][hit].astype(bool)
        p = G.fma32(d, t[:, None], o)
        c = scene_surface_colour(desc, leaf_model, inst, prim, u, v)
        if h:
            c = prod * c
        model = leaf_model[inst]
        wo = np.zeros_like(d); go = np.zeros(len(live), bool); light = np.zeros(len(live), bool)
        for mi in np.unique(model):
            sel = model == mi
            mat = desc.models[int(mi)].material
            w, followed, _ = G.follow_dir(mat.kind, mat.ior, d[sel], nrm[sel], front[sel])
            wo[sel] = w; go[sel] = followed & (h < max_hops)
            light[sel] = mat.kind == EMISSIVE
        e = ~go
        lm, mapped = scene_lookup(desc, maps, inst[e], prim[e], u[e], v[e])
        usable = mapped.astype(bool) & front[e]
        factor = np.where(usable[:, None], lm, unlit[None, :]).astype(F)
        b = np.where(light[e][:, None], c[e], c[e] * factor).astype(F)
        B[live[e]] = b
        ending[live[e]] = np.where(light[e], LIGHT, np.where(usable, MAPPED_FRONT, np.where(mapped.astype(bool), MAPPED_BACK, UNMAPPED)))
        live, o, d, prod = live[go], p[go], wo[go], c[go]
    assert (ending >= 0).all() and B.dtype == F
    return B, ending


def fold(samples):
    """the baked sums of per-sample B [k][rows, w, 3] in sample order: S.rgb += B, S.w += 1, binary32"""
    total = np.zeros(samples[0].shape[:2] + (4,), F)
    for b in samples:
        total = total + np.concatenate([b, np.ones(b.shape[:2] + (1,), F)], axis=2)
    assert total.dtype == F
    return total


# --------------------------------------------------------------------------------------------------------------------------------- scenes
def soup_scene(n_tris=40, seed=11):
    """a random-UV triangle soup as ONE model under three general rigid matrices (two get different 5 x 3 and 8 x 8 maps, the third none), and
    a second model without UVs; UVs reach far outside [0, 1] on every side"""
    rng = np.random.default_rng(seed)
    pos, nrm = LC._soup(n_tris, seed)
    uvs = rng.uniform(-0.6, 1.6, (n_tris, 3, 2)).astype(F)
    mats = np.stack([scenes.rigid_from_quat(1, -7, -3, 2, (3.0, -2.0, 1.0)), scenes.rigid_from_quat(3, -1, 2, 4, (-8.0, 0.5, 2.0)),
                     scenes.rigid_from_quat(2, 3, -5, 7, (0.0, 9.0, -4.0))]).astype(F)
    models = [Model.new(LC.QUAD_POS, LC.QUAD_NRM, Lambertian.new((0.5, 0.5, 0.5)), None, "plain"),
              Model.new(pos, nrm, Lambertian.new((0.8, 0.8, 0.8)), mats, "soup", uvs=uvs)]
    maps = {(1, 0): rng.uniform(0.0, 1.0, (3, 5, 3)).astype(F), (1, 1): rng.uniform(0.0, 1.0, (8, 8, 3)).astype(F)}
    return SceneDesc.new(models, None, "uv soup"), maps


def offset_scene(seed=13):
    """ONE triangle without UVs as the first model, then two mapped soups, the first under two matrices: in an untextured scene the device's
    compact UV table then starts exactly one triangle below each soup's first triangle in the flattened scene, the offset at which a
    leaf's way to its UVs is the all-ones word.  Every placement of the soups gets a map of its own."""
    rng = np.random.default_rng(seed)
    one_p, one_n = LC._soup(1, seed)
    models = [Model.new(one_p, one_n, Lambertian.new((0.5, 0.5, 0.5)), None, "one")]
    two = np.stack([scenes.rigid_from_quat(1, -7, -3, 2, (3.0, -2.0, 1.0)), scenes.rigid_from_quat(3, -1, 2, 4, (-8.0, 0.5, 2.0))]).astype(F)
    for name, n_tris, mats in (("first", 23, two), ("second", 9, None)):
        pos, nrm = LC._soup(n_tris, seed + n_tris)
        models.append(Model.new(pos, nrm, Lambertian.new((0.8, 0.8, 0.8)), mats, name, uvs=rng.uniform(-0.2, 1.2, (n_tris, 3, 2)).astype(F)))
    maps = {(1, 0): rng.uniform(0.0, 1.0, (3, 5, 3)).astype(F), (1, 1): rng.uniform(0.0, 1.0, (8, 8, 3)).astype(F),
            (2, 0): rng.uniform(0.0, 1.0, (16, 16, 3)).astype(F)}
    return SceneDesc.new(models, Camera.new((0.0, 0.0, 14.0), (0.0, 0.0, 0.0), 60.0, 48 / 32), "one triangle in front"), maps


def offset_queries(desc, n=300, seed=14):
    """random hits on offset_scene's four leaves (leaf 0 is the single triangle)"""
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, 4, n).astype(np.uint32)
    tris = np.array([desc.models[m].positions.shape[0] for m, _ in leaf_keys(desc)])
    prim = (rng.integers(0, 1 << 20, n) % tris[inst]).astype(np.uint32)
    u = rng.uniform(0, 1, n).astype(F)
    v = (rng.uniform(0, 1, n) * (1 - u)).astype(F)
    return inst, prim, u, v


def soup_queries(desc, n=777, seed=12):
    """random hits on soup_scene's four leaves (leaf 0 is the plain quad), more than one block and no multiple of it; the first queries pin
    the clamp on all four sides and at the corners through triangles whose UVs were replaced by far-out ones"""
    rng = np.random.default_rng(seed)
    inst = rng.integers(0, 4, n).astype(np.uint32)
    prim = np.where(inst == 0, rng.integers(0, 2, n), rng.integers(0, desc.models[1].positions.shape[0], n)).astype(np.uint32)
    u = rng.uniform(0, 1, n).astype(F)
    v = (rng.uniform(0, 1, n) * (1 - u)).astype(F)
    return inst, prim, u, v


CLAMP_UVS = [(-3.0, 0.4), (4.0, 0.4), (0.4, -3.0), (0.4, 4.0), (-3.0, -3.0), (4.0, -3.0), (-3.0, 4.0), (4.0, 4.0), (-1e30, 1e30), (0.0, 1.0), (1.0, 0.0)]


def clamp_scene():
    """one model whose triangle k has the single UV CLAMP_UVS[k] at all three vertices: the lookup's clamp on every side and corner"""
    k = len(CLAMP_UVS)
    pos, nrm = LC._soup(k, 5)
    uvs = np.array([[c, c, c] for c in CLAMP_UVS], F)
    return SceneDesc.new([Model.new(pos, nrm, Lambertian.new((0.8, 0.8, 0.8)), None, "clamp", uvs=uvs)], None, "clamp")


def centre_scene(w, h):
    """one model with a triangle per texel of a w x h map, all three UVs at that texel's centre ((i + .5) / w, (j + .5) / h)"""
    pos, nrm = LC._soup(w * h, 6)
    s = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    t = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    c = np.stack(np.meshgrid(s, t), axis=2).reshape(-1, 2).astype(F)
    return SceneDesc.new([Model.new(pos, nrm, Lambertian.new((0.8, 0.8, 0.8)), None, "centres", uvs=np.repeat(c[:, None, :], 3, axis=1))], None, "centres")


def _quad_uv():
    return LC.QUAD_UV.copy()          # G._quad's two triangles (a b c), (a c d): the unit square over the quad


MAPPED_MODELS = ["light", "lamp", "back", "behind", "panel", "tile", "floor", "mirror", "sky_mirror", "slab"]


def mapped_room(w=G.W, h=G.H):
    """An open room for the baked view, seen from (0, 0, 12) towards -z:
      lamp        an emissive quad in view, in front of the back wall (its emitted length is below 100); light: a larger one overhead
      back        the Lambertian back wall, mapped 16 x 16; behind: the wall behind the camera, mapped 5 x 3, seen only in the mirror
      panel       ONE mapped model of two quads side by side whose vertex normals face the camera on one and away from it on the other:
                  a mapped leaf seen from both faces
      tile        one quad under two general rigid matrices; only ordinal 1 gets a map
      floor       GGX metal without UVs: unmapped
      mirror      a flat mirror that shows `behind`; sky_mirror: one tilted upwards, whose chains leave the room: a miss after a hop
      slab        a glass pane in front of the back wall
    Every model but the two lights stands under a general rigid instance matrix.  Returns (scene, {(model, ordinal): map})."""
    glass = Dielectric.new((0.9, 0.95, 1.0), 1.5, None)
    parts = []
    lp, ln = G._quad((-6.0, 12.0, -6.0), (6.0, 12.0, -6.0), (6.0, 12.0, 6.0), (-6.0, 12.0, 6.0))
    parts.append(Model.new(lp.astype(F), ln.astype(F), Emissive.new((12.0, 11.0, 9.0)), None, "light"))
    mp, mn = G._quad((0.0, 3.0, -8.5), (6.0, 3.0, -8.5), (6.0, 7.0, -8.5), (0.0, 7.0, -8.5))
    parts.append(Model.new(mp.astype(F), mn.astype(F), Emissive.new((6.0, 5.0, 4.0)), None, "lamp"))
    parts.append(G._placed(*G._quad((-30.0, -20.0, -20.0), (30.0, -20.0, -20.0), (30.0, 25.0, -20.0), (-30.0, 25.0, -20.0)),
                           Lambertian.new((0.7, 0.7, 0.7)), (1, -7, -3, 2), "back", uvs=_quad_uv()))
    parts.append(G._placed(*G._quad((30.0, -20.0, 20.0), (-30.0, -20.0, 20.0), (-30.0, 30.0, 20.0), (30.0, 30.0, 20.0)),
                           Lambertian.new((0.9, 0.8, 1.0)), (3, -1, 2, 4), "behind", uvs=_quad_uv() * F(1.5) - F(0.25)))
    pa, na = G._quad((2.0, -5.5, -6.0), (6.0, -5.5, -6.0), (6.0, 2.5, -6.0), (2.0, 2.5, -6.0))
    pb, nb = G._quad((6.5, -5.5, -6.0), (12.0, -5.5, -6.0), (12.0, 2.5, -6.0), (6.5, 2.5, -6.0))
    panel_uv = np.concatenate([_quad_uv() * F(0.5), _quad_uv() * F(0.5) + F(0.5)])
    parts.append(G._placed(np.concatenate([pa, pb]), np.concatenate([na, -nb]), Lambertian.new((0.6, 0.9, 0.5)), (5, 1, 1, 7), "panel", uvs=panel_uv))
    # (ordinal 0 at (-4..-2, 2.5..4.5, -8); ordinal 1 is the same turn with another translation: the quad moved by (3.5, -6.5, 3))
    tile = G._placed(*G._quad((-4.0, 2.5, -8.0), (-2.0, 2.5, -8.0), (-2.0, 4.5, -8.0), (-4.0, 4.5, -8.0)), Lambertian.new((0.9, 0.5, 0.4)), (3, -1, 2, 4), "tile",
                     uvs=_quad_uv())
    tile.matrices = np.stack([tile.matrices[0], scenes.rigid_from_quat(3, -1, 2, 4, translation=(3.0 + 3.5, -2.0 - 6.5, 1.0 + 3.0))]).astype(F)
    parts.append(tile)
    parts.append(G._placed(*G._quad((-12.0, -6.0, 8.0), (12.0, -6.0, 8.0), (12.0, -6.0, -20.0), (-12.0, -6.0, -20.0)),
                           GGX.new_metal((0.9, 0.6, 0.2), 0.05), (2, 3, -5, 7), "floor"))
    parts.append(G._placed(*G._quad((-9.0, -2.0, -12.0), (-4.0, -2.0, -12.0), (-4.0, 4.0, -12.0), (-9.0, 4.0, -12.0)),
                           Specular.new((0.9, 0.8, 0.7)), (2, 3, -5, 7), "mirror"))
    parts.append(G._placed(*G._quad((-16.0, -4.0, -8.0), (-11.0, -4.0, -8.0), (-11.0, -1.0, -11.0), (-16.0, -1.0, -11.0)),
                           Specular.new((0.95, 0.95, 0.9)), (1, -7, -3, 2), "sky_mirror"))
    parts.append(G._placed(*G._box((-3.0, -4.0, -10.0), (1.0, 0.0, -9.0)), glass, (1, -7, 2, 3), "slab"))
    assert [m.name for m in parts] == MAPPED_MODELS
    rng = np.random.default_rng(21)
    name = MAPPED_MODELS.index
    maps = {(name("back"), 0): rng.uniform(0.0, 1.0, (16, 16, 3)).astype(F), (name("behind"), 0): rng.uniform(0.0, 1.0, (3, 5, 3)).astype(F),
            (name("panel"), 0): rng.uniform(0.0, 1.0, (3, 5, 3)).astype(F), (name("tile"), 1): rng.uniform(0.0, 1.0, (16, 16, 3)).astype(F)}
    cam = Camera.new((0.0, 0.0, 12.0), (0.0, -1.0, -2.0), 70.0, w / h)
    return SceneDesc.new(parts, cam, "mapped room"), maps


LIT_ALBEDO = 0.7


def lit_room(w=48, h=32):
    """A closed Lambertian room (albedo 0.7, a box seen from inside, box-atlas UVs), a Lambertian box on its floor under a general rigid
    matrix (box-atlas UVs too) and a small light without UVs under the ceiling; the camera is inside and every camera ray ends on a
    surface.  Returns (scene, the mapped placements [(model, ordinal)])."""
    rp, rn = box((-5.0, -4.0, -6.0), (5.0, 4.0, 6.0))
    room = Model.new(rp, (-rn).astype(F), Lambertian.new((LIT_ALBEDO,) * 3), None, "room", uvs=LC.box_atlas(rp))
    bp, bn = box((-3.0, -4.0, -3.5), (-0.5, -1.5, -1.0))
    crate = G._placed(bp.astype(np.float64), bn.astype(np.float64), Lambertian.new((0.7, 0.6, 0.5)), (1, -7, -3, 2), "crate", uvs=LC.box_atlas(bp))
    lp, ln = G._quad((-1.0, 3.9, -1.0), (1.0, 3.9, -1.0), (1.0, 3.9, 1.0), (-1.0, 3.9, 1.0))          # facing down
    light = Model.new(lp.astype(F), ln.astype(F), Emissive.new((20.0, 18.0, 15.0)), None, "light")
    cam = Camera.new((1.5, 0.0, 5.0), (-1.0, -1.5, -2.0), 65.0, w / h)
    return SceneDesc.new([room, crate, light], cam, "lit room"), [(0, 0), (1, 0)]


def luminance(rgb):
    rgb = np.asarray(rgb, np.float64)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]
