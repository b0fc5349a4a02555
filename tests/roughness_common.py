"""Shared by tests/test_roughness_host.py and tests/test_gpu_roughness.py: the definition of the GGX alpha at a hit under a roughness map
(include/pt_api.h, pt_set_material_roughness_texture) restated in numpy, every product, sum and difference ONE np.float32 operation in the
order the header writes them, and the scenes the tests use.  Nothing here calls the library or the device."""
import dataclasses

import numpy as np

import baked_common as BC
import guides_follow_common as G
import probe_depth_common as PD
import probe_grid_common as PG
import probe_radiance_common as PR
from normalmap_common import bilinear_const, general_turn
from path_tracer_amd.scene_desc import EMISSIVE, GGX, GGX_DIELECTRIC, GGX_METAL, IDENTITY_3x4, Emissive, Lambertian, Material, Model, SceneDesc, Texture
from textures_common import F, bilinear, box, corner_scene, quad, surface_colour, world_instance_models

GGX_KINDS = (GGX_METAL, GGX_DIELECTRIC)


# ---------------------------------------------------------------------------------------------------------------------------- the definition
def clamp_alpha(x):
    """alpha = x < 1e-4f ? 1e-4f : (x > 0.9999f ? 0.9999f : x), the expression pt_add_material applies to roughness * roughness"""
    x = np.asarray(x, F)
    return np.where(x < F(1e-4), F(1e-4), np.where(x > F(0.9999), F(0.9999), x)).astype(F)


def hit_st(uv3, u, v):
    """the surface colour's s, t: the hit's interpolated, repeat-addressed UV; uv3 [n, 3, 2] the hit triangles' UVs (load order)"""
    u = np.asarray(u, F); v = np.asarray(v, F); uv3 = np.asarray(uv3, F)
    st = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in (0, 1):
            a, b, c = uv3[:, 0, k], uv3[:, 1, k], uv3[:, 2, k]
            x = (a + u * (b - a)) + v * (c - a)
            st.append(x - np.floor(x))
    return st[0], st[1]


def hit_rho(tex, uv3, u, v):
    """rho [n] of hits under the roughness map tex [h, w, 3]: the first component of the normal map's lookup; g and b are not read"""
    s, t = hit_st(uv3, u, v)
    rho = bilinear_const(tex, s, t)[:, 0]
    assert rho.dtype == F
    return rho


def hit_alpha(tex, uv3, u, v):
    rho = hit_rho(tex, uv3, u, v)
    x = rho * rho
    assert x.dtype == F
    return clamp_alpha(x)


def material_alpha(roughness):
    """the stored alpha of a GGX material: clamp(sq(f32 roughness))"""
    r = F(roughness)
    return clamp_alpha(r * r)


def _per_model(desc, instance, prim, u, v, mapped, unmapped, other):
    instance = np.asarray(instance); prim = np.asarray(prim)
    u = np.asarray(u, F); v = np.asarray(v, F)
    out = np.zeros(len(instance), F)
    models = world_instance_models(desc)[instance]
    for mi in np.unique(models):
        sel = np.nonzero(models == mi)[0]
        mod = desc.models[int(mi)]
        mat = mod.material
        if mat.kind not in GGX_KINDS:
            out[sel] = other
        elif mat.roughness_texture is None:
            out[sel] = unmapped(mat)
        else:
            uv = np.asarray(mod.uvs, F) if mod.uvs is not None else np.zeros((mod.positions.shape[0], 3, 2), F)
            out[sel] = mapped(mat.roughness_texture.data, uv[prim[sel]], u[sel], v[sel])
    return out


def scene_alpha(desc, instance, prim, u, v):
    """the restated pt_surface_roughness of hits on a scene description: the alpha at the hit, the stored alpha of an unmapped GGX material,
    0 for a kind that is not GGX"""
    return _per_model(desc, instance, prim, u, v, hit_alpha, lambda m: material_alpha(m.roughness), F(0.0))


def scene_rho(desc, instance, prim, u, v):
    """the LINEAR roughness of the same hits (the material's own where there is no map, 0 off GGX): what an untextured material that shades
    the hit alike is made with"""
    return _per_model(desc, instance, prim, u, v, hit_rho, lambda m: F(m.roughness), F(0.0))


# ---------------------------------------------------------------------------------------------------------------------------------- scenes
def varied_map(w, h, seed, lo=0.1, hi=0.9):
    """w x h texels whose r values are distinct roughnesses in [lo, hi]; g and b hold other values, which nothing may read"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 3.0, (h, w, 3)).astype(F)
    r = np.linspace(lo, hi, w * h)
    rng.shuffle(r)
    t[..., 0] = r.reshape(h, w).astype(F)
    assert len(np.unique(t[..., 0])) == w * h
    return Texture.new(t)


def constant_map(w, h, rho):
    t = np.full((h, w, 3), 7.0, F)
    t[..., 0] = F(rho)
    t[..., 1] = F(0.25)
    return Texture.new(t)


UNMAPPED_ROUGHNESS = 0.37


def hook_scene(t53=None):
    """the unit hook's scene, modelled on normalmap_common.hook_scene: a GGX-metal box under a 5 x 3 map, placed twice (identity and a general
    rigid turn), with mirrored, degenerate, negative, exactly-1 and 1e6 UVs; a GGX-dielectric quad WITHOUT UVs under a 1 x 1 map; a light; a GGX
    box that is colour-textured and roughness-mapped (8 x 4); an unmapped GGX quad; a Lambertian quad.  t53: the first model's map"""
    rng = np.random.default_rng(11)
    t53 = varied_map(5, 3, 1) if t53 is None else t53
    t11 = Texture.new(np.array([[[0.55, 0.0, 9.0]]], F))
    d84 = varied_map(8, 4, 2).data.copy()
    d84[:, :3, 0] = F(0.005)                                                         # both clamps are reached: columns whose square is below
    d84[:, 5:, 0] = np.linspace(1.0, 1.2, 12).reshape(4, 3).astype(F)                # 1e-4 and columns whose square is above 0.9999
    t84 = Texture.new(d84)
    colour = Texture.new(rng.uniform(0.1, 0.9, (2, 2, 3)).astype(F))
    bp, bn = box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    uv = rng.uniform(-3.0, 3.0, (12, 3, 2)).astype(F)
    uv[0] = [[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]                                   # exactly 1.0
    uv[1] = [[-0.5, -2.0], [-1.0, -0.25], [-1e-9, -3.0]]                           # negative
    uv[2] = [[1.0e6, 1.0e6 + 0.5], [1.0e6 + 3.0, 999999.25], [1000001.5, 1.0e6]]   # around 1e6
    uv[3] = [[0.2, 0.4], [0.2, 0.4], [0.2, 0.4]]                                   # degenerate: all equal
    uv[4] = [[0.1, 0.1], [0.3, 0.3], [0.7, 0.7]]                                   # degenerate: collinear
    uv[5] = [[0.1, 0.2], [0.9, 0.3], [0.4, 0.8]]
    uv[6] = uv[5][[0, 2, 1]]                                                       # ... and its mirror image on the next triangle
    two = np.stack([IDENTITY_3x4, IDENTITY_3x4]).astype(F)
    two[1] = general_turn()
    two[1, :, 3] = (5.0, 0.5, -1.0)
    qp, qn = quad((-9.0, -2.0, -9.0), (-9.0, -2.0, 9.0), (9.0, -2.0, 9.0), (9.0, -2.0, -9.0))
    lp, ln = quad((-1.0, 8.0, -1.0), (1.0, 8.0, -1.0), (1.0, 8.0, 1.0), (-1.0, 8.0, 1.0))
    models = [
        Model.new(bp, bn, GGX.new_metal((0.8, 0.6, 0.4), 0.3).roughness_mapped(t53), two, "instanced", uvs=uv),
        Model.new(qp, qn, GGX.new_dielectric((1.0, 1.0, 1.0), 0.4, 1.5).roughness_mapped(t11), None, "no uvs"),
        Model.new(lp, ln, Emissive.new((5.0, 5.0, 5.0)), None, "light"),
        Model.new(bp + F(20.0), bn, GGX.new_metal((0.3, 0.9, 0.5), 0.2).textured(colour).roughness_mapped(t84), None, "eight by four",
                  uvs=rng.uniform(0.0, 1.0, (12, 3, 2)).astype(F)),
        Model.new(qp + F(0.5), qn, GGX.new_metal((0.1, 0.2, 0.3), UNMAPPED_ROUGHNESS), None, "unmapped", uvs=rng.uniform(0.0, 1.0, (2, 3, 2)).astype(F)),
        Model.new(qp + F(1.0), qn, Lambertian.new((0.1, 0.2, 0.3)), None, "lambertian", uvs=rng.uniform(0.0, 1.0, (2, 3, 2)).astype(F)),
    ]
    return SceneDesc.new(models, None, "surface roughness")


def untextured(desc):
    """the description with no texture of any kind on any material"""
    def strip(m):
        if m.kind == EMISSIVE:
            return m.emission_textured(None)
        m = m.textured(None).normal_mapped(None)
        return m.roughness_mapped(None) if m.kind in GGX_KINDS else m
    return SceneDesc.new([dataclasses.replace(m, material=strip(m.material), uvs=None) for m in desc.models], desc.camera, "no texture at all")


def hook_queries(desc, n=3000):
    """seeded hits {world instance, load-order primitive, u, v} on every model of a description; the vertices and an edge, and, where model 0
    is the instanced box, every special triangle of it through both instances"""
    rng = np.random.default_rng(8)
    inst_model = world_instance_models(desc)
    inst = rng.integers(0, len(inst_model), n).astype(np.uint32)
    ntri = np.array([desc.models[m].positions.shape[0] for m in inst_model])[inst]
    prim = (rng.integers(0, 1 << 30, n) % ntri).astype(np.uint32)
    u = rng.uniform(0.0, 1.0, n).astype(F)
    v = (rng.uniform(0.0, 1.0, n).astype(F) * (F(1.0) - u)).astype(F)
    u[:6] = [0.0, 1.0, 0.0, 0.5, 0.25, 1.0]; v[:6] = [0.0, 0.0, 1.0, 0.5, 0.75, 0.0]
    if desc.models[0].positions.shape[0] >= 7 and desc.models[0].matrices.shape[0] == 2:
        inst[6:20] = [0, 1] * 7; prim[6:20] = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    return inst, prim, u, v


# ---- the texel-corner room (textures_common.corner_scene) under ONE shared 2 x 2 roughness map on its metal and on its glass
R22 = {(0, 0): 0.15, (1, 0): 0.55, (1, 1): 0.3, (0, 1): 0.8}                         # all differ from the materials' own 0.35 and 0.2


def corner_map():
    t = np.zeros((2, 2, 3), F)
    for (i, j), r in R22.items():
        t[j, i] = (r, 1.0 - r, 5.0 + r)                                              # g and b hold other values
    return Texture.new(t)


def equivalent(desc):
    """the untextured description the definition makes equal to `desc`, for descriptions whose models carry ONE texel corner each (constant
    UVs at (i / w, j / h), w and h powers of two): every model gets a material of its own with colour f32(tint * texel) and the texel's r as
    roughness.  Computed through the restatement at the model's UV, which is exact there."""
    out = []
    z = np.zeros(1, F)
    for m in desc.models:
        mat = m.material
        if mat.kind == EMISSIVE:
            out.append(dataclasses.replace(m, uvs=None))
            continue
        uv = np.asarray(m.uvs, F)[:1] if m.uvs is not None else np.zeros((1, 3, 2), F)
        col = surface_colour(mat.colour, None if mat.texture is None else mat.texture.data, uv, z, z)[0]
        rough = mat.roughness
        if mat.roughness_texture is not None:
            rough = float(hit_rho(mat.roughness_texture.data, uv, z, z)[0])
        out.append(dataclasses.replace(m, material=Material(mat.kind, tuple(float(c) for c in col), rough, mat.ior, mat.volume), uvs=None))
    return SceneDesc.new(out, desc.camera, "untextured equivalent")


def with_roughness(desc, rmap, kinds=GGX_KINDS, keep_colour=True, normal=None):
    """`desc` with rmap on every material of `kinds`; keep_colour False strips the colour textures; normal: a normal map for every surface"""
    def f(m):
        if m.kind == EMISSIVE:
            return m
        if not keep_colour:
            m = m.textured(None)
        if normal is not None:
            m = m.normal_mapped(normal)
        return m.roughness_mapped(rmap) if m.kind in kinds else m
    return SceneDesc.new([dataclasses.replace(m, material=f(m.material)) for m in desc.models], desc.camera, desc.name if hasattr(desc, "name") else "")


def corner_room(width, height, media=True, lens=False, keep_colour=True, normal=None):
    """(roughness-mapped description, its untextured equivalent)"""
    tex, _ = corner_scene(width, height, lens=lens, media=media)
    mapped = with_roughness(tex, corner_map(), keep_colour=keep_colour, normal=normal)
    return mapped, equivalent(mapped)


def random_uv_room(width, height, rho=0.45):
    """the room without media, a constant 4 x 2 map of rho on its metal, and every model's UVs random in [-2, 3]; the colour textures are
    stripped (their texels vary).  Returns (description, the room with roughness rho on its metal)"""
    tex, _ = corner_scene(width, height, media=False)
    rng = np.random.default_rng(31)
    mapped = with_roughness(tex, constant_map(4, 2, rho), kinds=(GGX_METAL,), keep_colour=False)
    mapped = SceneDesc.new([dataclasses.replace(m, uvs=rng.uniform(-2.0, 3.0, (m.positions.shape[0], 3, 2)).astype(F)) for m in mapped.models], mapped.camera, "constant map")
    plain = []
    for m in untextured(mapped).models:
        mat = m.material
        if mat.kind == GGX_METAL:
            mat = Material(mat.kind, mat.colour, float(F(rho)), mat.ior, mat.volume)
        plain.append(dataclasses.replace(m, material=mat))
    return mapped, SceneDesc.new(plain, mapped.camera, "roughness rho")


# ---- the baked view's metal ending with the alpha at the hit
def baked(orc, desc, maps, grid, depth, rad, o, d, max_hops, unlit=(0.0, 0.0, 0.0), mapped=True):
    """probe_radiance_common.baked with ONE change: the alpha handed to the specular lookup is the restated alpha at the hit (scene_alpha)
    where mapped, the material's own where not.  Returns (B [n, 3], ending [n], on_metal [n], alpha [n]: the alpha of a chain that ended on
    GGX metal, 0 elsewhere)"""
    o = np.asarray(o, F).reshape(-1, 3).copy(); d = np.asarray(d, F).reshape(-1, 3).copy()
    n = o.shape[0]
    unlit = np.asarray(unlit, F)
    leaf_model = world_instance_models(desc)
    look = desc if mapped else untextured_roughness(desc)
    B = np.zeros((n, 3), F); ending = np.full(n, -1, np.int64); on_metal = np.zeros(n, bool); end_alpha = np.zeros(n, F)
    live = np.arange(n)
    prod = None
    for h in range(max_hops + 1):
        if live.size == 0:
            break
        tc = orc.trace_closest(o, d)
        hit = tc["inst"] != PG.MISS
        miss = live[~hit]
        B[miss] = BC.AMBIENT if prod is None else prod[~hit] * BC.AMBIENT
        ending[miss] = PG.MISS_AFTER_HOPS if h else PG.MISS_AT_0
        live, o, d = live[hit], o[hit], d[hit]
        if prod is not None:
            prod = prod[hit]
        inst, prim, t = tc["inst"][hit], tc["prim"][hit], tc["t"][hit]
        u, v = tc["u"][hit], tc["v"][hit]
        nrm, front = tc["normal"][hit], tc["front"][hit].astype(bool)
        p = G.fma32(d, t[:, None], o)
        from textures_common import scene_surface_colour
        c = scene_surface_colour(desc, leaf_model, inst, prim, u, v)
        if h:
            c = prod * c
        model = leaf_model[inst]
        wo = np.zeros_like(d); go = np.zeros(len(live), bool); light = np.zeros(len(live), bool)
        metal = np.zeros(len(live), bool)
        for mi in np.unique(model):
            sel = model == mi
            mat = desc.models[int(mi)].material
            w, followed, _ = G.follow_dir(mat.kind, mat.ior, d[sel], nrm[sel], front[sel])
            wo[sel] = w; go[sel] = followed & (h < max_hops)
            light[sel] = mat.kind == EMISSIVE
            metal[sel] = mat.kind == GGX_METAL
        alpha = scene_alpha(look, inst, prim, u, v)                                 # THE change: per hit
        e = ~go
        lm, is_mapped = BC.scene_lookup(desc, maps, inst[e], prim[e], u[e], v[e])
        is_mapped = is_mapped.astype(bool)
        usable = is_mapped & front[e]
        irr, lit = PD.lookup(grid, depth, p[e], nrm[e])
        lit = lit.astype(bool)
        spec, slit = PR.specular(grid, depth, rad, p[e], nrm[e], d[e], alpha[e])
        shiny = metal[e] & slit.astype(bool)
        on_metal[live[e]] = metal[e]
        end_alpha[live[e]] = np.where(metal[e], alpha[e], F(0.0))
        factor = np.where(usable[:, None], lm, np.where(lit[:, None], irr, unlit[None, :])).astype(F)
        factor = np.where(shiny[:, None], spec, factor).astype(F)
        b = np.where(light[e][:, None], c[e], c[e] * factor).astype(F)
        B[live[e]] = b
        other = np.where(is_mapped, np.where(lit, PG.PROBE_BACK, PG.UNLIT_BACK), np.where(lit, PG.PROBE_UNMAPPED, PG.UNLIT_UNMAPPED))
        kind = np.where(light[e], PG.LIGHT, np.where(usable, PG.MAPPED_FRONT, other))
        ending[live[e]] = np.where(shiny, np.where(front[e], PR.METAL_FRONT, PR.METAL_BACK), kind)
        live, o, d, prod = live[go], p[go], wo[go], c[go]
    assert (ending >= 0).all() and B.dtype == F
    return B, ending, on_metal, end_alpha


def untextured_roughness(desc):
    """the description without its roughness maps (everything else stays)"""
    return SceneDesc.new([dataclasses.replace(m, material=m.material.roughness_mapped(None) if m.material.kind in GGX_KINDS else m.material)
                          for m in desc.models], desc.camera, "no roughness map")


__all__ = ["F", "bilinear"]
