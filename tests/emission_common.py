"""Shared by tests/test_emission_textures_host.py and tests/test_gpu_emission_textures.py: the definition of emission textures
(include/pt_api.h: EMITTED COLOUR, LIGHT WEIGHT) restated in numpy over tests/textures_common.py's restatement of the surface colour, every
operation ONE np.float32 operation in the order the header writes them, and the scenes the tests render.  Nothing here calls the library."""
import numpy as np

from path_tracer_amd import scenes
from path_tracer_amd.scene_desc import EMISSIVE, IDENTITY_3x4, Camera, Emissive, Lambertian, Model, SceneDesc, Specular, Texture
from textures_common import F, LOUD, box, const_uvs, corner_scene, quad, surface_colour, world_instance_models

CENTROID = F(0.33333334)                                   # the barycentrics of the light weight's one-point quadrature


def material_texture(mat):
    """the texture the surface colour of a material is looked up in: its emission texture for an emissive one"""
    return mat.emission_texture if mat.kind == EMISSIVE else mat.texture


def scene_colour(desc, instance_model, instance, prim, u, v):
    """the restated surface / emitted colour of hits on a scene description: instance_model[i] = model of world instance i"""
    instance = np.asarray(instance); prim = np.asarray(prim)
    out = np.zeros((len(instance), 3), F)
    models = np.asarray(instance_model)[instance]
    for mi in np.unique(models):
        sel = np.nonzero(models == mi)[0]
        mod = desc.models[int(mi)]
        tex = material_texture(mod.material)
        uv = mod.uvs if mod.uvs is not None else np.zeros((mod.positions.shape[0], 3, 2), F)
        out[sel] = surface_colour(mod.material.colour, None if tex is None else tex.data, uv[prim[sel]], np.asarray(u, F)[sel], np.asarray(v, F)[sel])
    return out


def len3(c):
    c = np.asarray(c, F)
    return np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])


def light_cdf(desc, n0_of):
    """LightSampler::new (light_sampler.rs:41-61) over the header's LIGHT WEIGHT: every emissive model in order, its triangles in load order,
    weight = area * len(emitted colour at CENTROID); n0_of(model, prim) = the triangle's unnormalised normal (area = 0.5 * its length,
    primitive.rs:94).  Returns pdf, cdf, max as the sampler holds them"""
    weights = []
    for mi, mod in enumerate(desc.models):
        if mod.material.kind != EMISSIVE:
            continue
        n = mod.positions.shape[0]
        tex = material_texture(mod.material)
        uv = mod.uvs if mod.uvs is not None else np.zeros((n, 3, 2), F)
        ec = surface_colour(mod.material.colour, None if tex is None else tex.data, uv, np.full(n, CENTROID, F), np.full(n, CENTROID, F))
        for p in range(n):
            area = F(0.5) * len3(np.asarray(n0_of(mi, p), F))
            weights.append(F(area * len3(ec[p])))
    total = F(0.0)
    for w in weights:
        total = F(total + w)
    pdf = np.array([F(w / total) for w in weights], F)
    cdf = np.zeros(len(weights), F)
    run = F(0.0)
    for i, p in enumerate(pdf):
        run = F(run + p)
        cdf[i] = run
    return pdf, cdf, total


# ---------------------------------------------------------------------------------------------------------------------------------- scenes
TINT = (0.9, 0.8, 0.7)
QUIET = {(0, 0): (14.0, 12.0, 9.0), (2, 0): (5.0, 9.0, 12.0), (3, 1): (10.0, 4.0, 8.0)}


def emission_texture_42():
    t = np.full((2, 4, 3), LOUD, F)
    for (i, j), c in QUIET.items():
        t[j, i] = c
    return t


def emission_corner_scene(width, height, media=True, wall_textures=True, corners=((0, 0), (2, 0), (3, 1))):
    """textures_common.corner_scene's room with its light replaced: three light models of different size on ONE emissive material with a
    4 x 2 emission texture — a wall lamp the camera sees, a small lamp under a general rigid instance, a ceiling lamp with two instances —
    each with all its vertices at its own quiet texel corner (the other texels are LOUD), an untextured light, and a mirror block whose top
    reflects the wall lamp.  wall_textures=False takes the walls' textures away: the emission texture is then the scene's only texture.
    Returns (textured description, the equivalent untextured one: every lamp with its own Emissive(f32(tint * texel)))."""
    tex, plain = corner_scene(width, height, media=media)
    walls_t = (tex if wall_textures else plain).models[1:]
    walls_p = plain.models[1:]
    e42 = emission_texture_42()
    lamp = Emissive.new(TINT).emission_textured(Texture.new(e42))
    S = 10.0
    two = np.stack([IDENTITY_3x4, IDENTITY_3x4]); two[1, :, 3] = (4.0, 0.0, 3.0)
    parts = [  # name, geometry, matrices
        ("lamp_wall", quad((-3.0, -4.0, -S + 0.05), (4.0, -4.0, -S + 0.05), (4.0, 1.0, -S + 0.05), (-3.0, 1.0, -S + 0.05)), None),
        ("lamp_turned", quad((-1.0, 0.0, -1.0), (1.0, 0.0, -1.0), (1.0, 0.0, 1.0), (-1.0, 0.0, 1.0)), scenes.rigid_from_quat(3, -1, 2, 4, (5.0, 4.0, 4.0))[None]),
        ("lamp_pair", quad((-7.0, S - 0.05, -1.0), (-5.5, S - 0.05, -1.0), (-5.5, S - 0.05, 0.5), (-7.0, S - 0.05, 0.5)), two),
    ]
    textured, untextured = [], []
    for (name, (p, n), mats), (i, j) in zip(parts, corners):
        textured.append(Model.new(p, n, lamp, mats, name, uvs=const_uvs(p.shape[0], i / 4, j / 2)))
        col = (np.asarray(TINT, F) * e42[j, i]).astype(F)
        untextured.append(Model.new(p, n, Emissive.new(tuple(float(c) for c in col)), mats, name))
    bp, bn = quad((6.0, S - 0.05, 5.0), (8.0, S - 0.05, 5.0), (8.0, S - 0.05, 7.0), (6.0, S - 0.05, 7.0))
    bare = Model.new(bp, bn, Emissive.new((3.0, 4.0, 6.0)), None, "bare")
    mp, mn = box((-0.5, -S, -5.0), (1.5, -4.0, -2.5))
    mirror = Model.new(mp, mn, Specular.new((0.9, 0.95, 1.0)), None, "mirror")
    cam = tex.camera
    return (SceneDesc.new(textured + [bare, mirror] + list(walls_t), cam, "emission corners"),
            SceneDesc.new(untextured + [bare, mirror] + list(walls_p), cam, "emission corners, untextured"))


N_LAMPS = 3            # models 0..2 of emission_corner_scene are the textured lamps, 3 the bare light, 4 the mirror
MIRROR = 4


def varying_light_scene(width, height):
    """A light whose UVs vary across its triangles (beyond [0, 1), negative) on a 5 x 3 emission texture of random texels, seen by the camera
    directly and from a grey Lambertian floor; a mirror block that shows the light; open to the sides (misses)."""
    rng = np.random.default_rng(11)
    tex = Texture.new(rng.uniform(0.5, 6.0, (3, 5, 3)).astype(F))
    lamp = Emissive.new((1.0, 0.8, 0.6)).emission_textured(tex)
    lp, ln = quad((-4.0, -2.0, -7.0), (5.0, -2.0, -7.0), (5.0, 5.0, -7.0), (-4.0, 5.0, -7.0))        # faces the camera (+z)
    l_uv = np.array([[[-1.25, 0.1], [0.7, -0.4], [1.9, 1.3]], [[-1.25, 0.1], [1.9, 1.3], [-0.3, 2.2]]], F)
    fp, fn = quad((-8.0, -4.0, -8.0), (-8.0, -4.0, 8.0), (8.0, -4.0, 8.0), (8.0, -4.0, -8.0))
    mp, mn = box((-6.5, -4.0, -3.0), (-4.0, 2.5, -1.0))                                            # its +x face shows the lamp
    models = [Model.new(lp, ln, lamp, None, "lamp", uvs=l_uv), Model.new(fp, fn, Lambertian.new((0.5, 0.5, 0.5)), None, "floor"),
              Model.new(mp, mn, Specular.new((1.0, 1.0, 1.0)), None, "mirror")]
    return SceneDesc.new(models, Camera.new((1.0, 1.5, 9.0), (0.0, 0.0, -2.0), 65.0, width / height), "varying uvs on a light")


# ---- the plumbing scene of the NEE-on test: explicit and BSDF estimate read the texture at (triangle, u, v)
def plumbing_texture():
    """8 x 8 texels that are exactly 0 or 8: four lit patches of 2 x 2 texels on black.  The bilinear lookup blends a texel with its right and
    lower neighbours, so a patch lights a 3 x 3-texel region and about half of the lamp reads exactly black; both triangles' centroids
    (s, t) = (2/3, 1/3) and (1/3, 2/3) read a lit patch, so both have a weight"""
    t = np.zeros((8, 8, 3), F)
    for i, j in ((0, 0), (2, 1), (1, 3), (3, 2)):                    # patch column, row
        t[2 * j:2 * j + 2, 2 * i:2 * i + 2] = 8.0
    return t


def plumbing_scene(width, height):
    """a white Lambertian floor under a large down-facing light quad whose UVs span an 8 x 8 emission texture; the camera looks down at the
    floor only"""
    lamp = Emissive.new((1.0, 1.0, 1.0)).emission_textured(Texture.new(plumbing_texture()))
    lp, ln = quad((-6.0, 3.0, -6.0), (6.0, 3.0, -6.0), (6.0, 3.0, 6.0), (-6.0, 3.0, 6.0))             # normal (0, -1, 0)
    l_uv = np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0]]], F)
    fp, fn = quad((-9.0, 0.0, -9.0), (-9.0, 0.0, 9.0), (9.0, 0.0, 9.0), (9.0, 0.0, -9.0))
    models = [Model.new(lp, ln, lamp, None, "lamp", uvs=l_uv), Model.new(fp, fn, Lambertian.new((1.0, 1.0, 1.0)), None, "floor")]
    return SceneDesc.new(models, Camera.new((0.0, 2.5, 0.5), (0.0, 0.0, 0.0), 80.0, width / height), "plumbing")


def fma32(a, b, c):
    """f32::mul_add: a * b + c rounded ONCE to binary32 (the product is exact in binary64; the sum is rounded to odd there)"""
    import math
    p = float(a) * float(b)
    c = float(c)
    s = p + c
    if math.isfinite(s):
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        if err != 0.0 and (np.float64(s).view(np.uint64) & np.uint64(1)) == 0:
            s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return F(s)


def plumbing_prediction(desc, orc, orc_white, cdf, width, height, spp, seed):
    """Per sample of plumbing_scene at max_bounces = 0: 0 predicted zero, 1 predicted nonzero, 2 excluded as ambiguous.
    Stream draws 1..3 give x, lu, lv; a binary search of `cdf` (the library's pt_light_cdf) gives the triangle; the restated lookup at
    (lu, lv) gives E_explicit; orc_white.material_eval(draws_consumed=4) gives wo; trace_closest(which=1) from r.at(t) gives the light hit and
    the lookup there E_bsdf.  Zero when both are exactly (0, 0, 0).  Excluded: a camera ray that does not end on the floor (the restated
    lookup is exact, and so are the coordinates it is given: nothing else is ambiguous)."""
    from materials_common import stream_f32
    lamp = desc.models[0]
    tex = lamp.material.emission_texture.data
    out = np.zeros((spp, height * width), np.uint8)

    for s in range(spp):
        draws = stream_f32(seed, np.arange(width * height), np.full(width * height, s), 1, 3)
        for p in range(width * height):
            o, d = orc.primary_ray(width, height, p, s)
            h = orc.trace_closest(o[None], d[None])
            if h["inst"][0] != 1:                                       # not the floor
                out[s, p] = 2
                continue
            x, lu, lv = draws[p]
            tri = min(int(np.searchsorted(cdf, x, side="left")), len(cdf) - 1)
            if lu + lv > F(1.0):
                lu, lv = F(1.0) - lu, F(1.0) - lv
            e_exp = surface_colour(lamp.material.colour, tex, lamp.uvs[tri][None], [lu], [lv])[0]
            ev = orc_white.material_eval(0, d, h["normal"][0], int(h["front"][0]), p, s, draws_consumed=4)
            wo = ev[0:3]
            at = np.array([fma32(d[k], h["t"][0], o[k]) for k in range(3)], F)
            lh = orc.trace_closest(at[None], wo[None], which=1)
            e_bsdf = np.zeros(3, F)
            if lh["inst"][0] != 0xFFFFFFFF:
                e_bsdf = surface_colour(lamp.material.colour, tex, lamp.uvs[lh["prim"][0]][None], [lh["u"][0]], [lh["v"][0]])[0]
            out[s, p] = int(bool(e_exp.any() or e_bsdf.any()))
    return out


def dim_scene(width, height):
    """the unbiasedness scene: a large dim light (emission <= 4) with a smooth-and-checkered emission texture over an albedo-0.5 floor and a
    back wall, open elsewhere"""
    i, j = np.meshgrid(np.arange(8), np.arange(8))
    lum = np.where((i + j) & 1, F(0.25), F(1.0)) * (F(1.0) + F(0.375) * i.astype(F))               # 0.25 .. 3.625
    t = np.stack([lum, lum * F(0.75), lum * F(0.5)], axis=2).astype(F)
    assert t.max() <= 4.0
    lamp = Emissive.new((1.0, 1.0, 1.0)).emission_textured(Texture.new(t))
    lp, ln = quad((-5.0, 5.0, -5.0), (5.0, 5.0, -5.0), (5.0, 5.0, 5.0), (-5.0, 5.0, 5.0))
    l_uv = np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0]]], F)
    fp, fn = quad((-8.0, 0.0, -8.0), (-8.0, 0.0, 8.0), (8.0, 0.0, 8.0), (8.0, 0.0, -8.0))
    bp, bn = quad((-8.0, 0.0, -8.0), (8.0, 0.0, -8.0), (8.0, 6.0, -8.0), (-8.0, 6.0, -8.0))
    grey = Lambertian.new((0.5, 0.5, 0.5))
    models = [Model.new(lp, ln, lamp, None, "lamp", uvs=l_uv), Model.new(fp, fn, grey, None, "floor"), Model.new(bp, bn, grey, None, "back")]
    return SceneDesc.new(models, Camera.new((0.0, 2.0, 9.0), (0.0, 1.0, 0.0), 60.0, width / height), "dim textured light")

