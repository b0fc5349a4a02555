"""numpy restatement of include/pt_api.h's pt_bake_lightmap_direct, every operation ONE np.float32 operation in the order the header writes
them, and the scenes its tests share.  Nothing here calls the library under test: stream draws are materials_common.stream_f32's, the light
table and the light triangles the oracle's (light_cdf, triangle; under an emission texture emission_common's restated weights over the
oracle's triangles), the shadow ray Oracle.trace_any, the gather radiance Oracle.integrate with the oracle's first-hit id, the rays
lightmap_common's and the fold lightmap_common.fold's rule applied to X."""
import numpy as np

import emission_common as EC
import lightmap_common as LC
from materials_common import stream_f32
from textures_common import surface_colour

F = np.float32
D64 = np.float64
SEED = LC.SEED
EMISSIVE = 1
DEPTH = 6


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- the light table
class LightTable:
    """pdf, cdf [L]; model [L] the scene's model of light i, prim [L] its load-order triangle; pos, nrm [L, 3, 3]; n0 [L, 3]"""

    def __init__(self, orc, desc):
        emissive = [i for i, m in enumerate(desc.models) if m.material.kind == EMISSIVE]
        c = orc.light_cdf()
        tri = np.array([orc.triangle(int(b), int(p), which=1) for b, p in zip(c["blas"], c["prim"])], F).reshape(-1, 36)
        self.model = np.array([emissive[int(b)] for b in c["blas"]], np.int64)
        self.prim = c["prim"].astype(np.int64)
        self.n0 = tri[:, 0:3].copy()
        self.pos = tri[:, 12:21].reshape(-1, 3, 3).copy()
        self.nrm = tri[:, 21:30].reshape(-1, 3, 3).copy()
        self.pdf, self.cdf = c["pdf"], c["cdf"]
        self.desc = desc
        if any(desc.models[i].material.emission_texture is not None for i in emissive):
            # the oracle knows no textures: the header's LIGHT WEIGHT restated (emission_common) over the oracle's triangles, in its order
            order = [(mi, p) for mi in emissive for p in range(desc.models[mi].positions.shape[0])]
            assert order == list(zip(self.model.tolist(), self.prim.tolist()))
            where = {mp: i for i, mp in enumerate(order)}
            self.pdf, self.cdf, _ = EC.light_cdf(desc, lambda mi, p: self.n0[where[(mi, p)]])
        assert self.pdf.dtype == F and self.cdf.dtype == F

    def emitted(self, i, lu, lv):
        """the emitted colour of light i[n] at barycentrics (lu, lv) [n] -> [n, 3]"""
        out = np.zeros((len(i), 3), F)
        for mi in np.unique(self.model[i]):
            sel = np.nonzero(self.model[i] == mi)[0]
            mod = self.desc.models[int(mi)]
            tex = mod.material.emission_texture
            uv = mod.uvs if mod.uvs is not None else np.zeros((mod.positions.shape[0], 3, 2), F)
            out[sel] = surface_colour(mod.material.colour, None if tex is None else tex.data, uv[self.prim[i][sel]], lu[sel], lv[sel])
        return out


def finalise(v):
    """the finite check and the length clamp of 100 every sample ends with"""
    v = np.array(v, F)
    v[~np.isfinite(v).all(1)] = 0
    l2 = _dot3(v, v)
    over = l2 > F(100.0) * F(100.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (F(1.0) / np.sqrt(l2)) * F(100.0)
    v[over] = v[over] * s[over, None]
    assert v.dtype == F
    return v


def light_samples(lt, keys, samples, o, n, seed=SEED):
    """THE LIGHT SAMPLE of the header, line for line, for streams (keys[i], samples[i]) at origins o [k, 3] under normals n [k, 3]:
    dict(light, dir, t_max, c, cast, ce (before the shadow ray; zeros without one), clamped)"""
    o = np.asarray(o, F); n = np.asarray(n, F)
    u = stream_f32(seed, np.asarray(keys, np.uint64), np.asarray(samples, np.uint64), 0, 3)
    x, lu, lv = u[:, 0], u[:, 1], u[:, 2]
    i = np.minimum(np.searchsorted(lt.cdf, x, side="left"), len(lt.cdf) - 1)        # entries below x (the cdf ascends, nothing is a NaN)
    flip = lu + lv > F(1.0)
    lu, lv = np.where(flip, F(1.0) - lu, lu), np.where(flip, F(1.0) - lv, lv)
    lw = F(1.0) - lu - lv
    A, B, C = lt.pos[i, 0], lt.pos[i, 1], lt.pos[i, 2]
    NA, NB, NC = lt.nrm[i, 0], lt.nrm[i, 1], lt.nrm[i, 2]
    point = (A * lw[:, None] + B * lu[:, None]) + C * lv[:, None]
    lnr = (NA * lw[:, None] + NB * lu[:, None]) + NC * lv[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ln = lnr / np.sqrt(_dot3(lnr, lnr))[:, None]
        w = point - o
        dist2 = _dot3(w, w)
        dist = np.sqrt(dist2)
        dr = w / dist[:, None]
        c = _dot3(dr, n)
        cast = c > 0
        sample_pdf = lt.pdf[i] / (F(0.5) * np.sqrt(_dot3(lt.n0[i], lt.n0[i])))
        cosl = np.abs(_dot3(dr, ln))
        light_pdf = sample_pdf * (dist2 / cosl)
        emitted = lt.emitted(i, lu, lv)
        raw = ((emitted * np.abs(c)[:, None]) * F(0.31830987)) / light_pdf[:, None]
    ce = finalise(raw)
    clamped = cast & np.isfinite(raw).all(1) & (_dot3(raw, raw) > F(100.0) * F(100.0))
    ce[~cast] = 0
    t_max = (F(1.0) - F(5e-4)) * dist
    for a in (point, ln, dr, c, ce, t_max, light_pdf):
        assert a.dtype == F
    return dict(light=i.astype(np.uint32), dir=dr, t_max=t_max, c=c, cast=cast, ce=ce, clamped=clamped)


def shadowed(orc, o, ls):
    """blocked [k] bool: TLAS::any_intersect over the world for the samples that cast a shadow ray"""
    blocked = np.zeros(len(ls["cast"]), bool)
    idx = np.nonzero(ls["cast"])[0]
    if len(idx):
        blocked[idx] = orc.trace_any(np.asarray(o, F)[idx], ls["dir"][idx], ls["t_max"][idx]) != 0
    return blocked


def emissive_ids(desc):
    """[256] bool: the first-hit id bytes (a model index's low byte) that mean an emissive model"""
    out = np.zeros(256, bool)
    for i, m in enumerate(desc.models):
        if m.material.kind == EMISSIVE:
            out[i & 0xFF] = True
    return out


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def bake_samples(O, orc, desc, table, n_samples, first_sample=0, key_base=0, light_key_base=None, bias=0.0, depth=DEPTH, nee=1):
    """every sample of a direct bake over a texel table, texel-major with a texel's samples consecutive: dict(k covered texel indices,
    X [c * n, 3], G, D, zeroed (the gather ray's first hit is a lamp), blocked, cast, plain (the gather radiance before the zeroing))"""
    h, w = table[0].shape
    if light_key_base is None:
        light_key_base = key_base + w * h
    k, o, d, keys, smp = LC.bake_rays(O, table, n_samples, first_sample, key_base, bias)
    nrm = np.repeat(table[3].reshape(-1, 3)[k], n_samples, 0)
    lt = LightTable(orc, desc)
    ls = light_samples(lt, np.repeat((k + light_key_base).astype(np.uint64), n_samples), smp, o, nrm)
    blocked = shadowed(orc, o, ls)
    Dl = np.where((blocked | ~ls["cast"])[:, None], F(0.0), ls["ce"]).astype(F)
    rad = np.zeros((len(keys), 3), F); ids = np.zeros(len(keys), np.int64)
    for i in range(len(keys)):
        col, _, ids[i] = orc.integrate(o[i], d[i], int(keys[i]), int(smp[i]), 1, max_bounces=depth, enable_nee=nee)
        rad[i] = col[:3]
    zeroed = emissive_ids(desc)[ids]
    G = np.where(zeroed[:, None], F(0.0), rad).astype(F)
    X = G + Dl
    assert X.dtype == F
    return dict(k=k, X=X, G=G, D=Dl, zeroed=zeroed, blocked=blocked, cast=ls["cast"], plain=rad, light=ls["light"], clamped=ls["clamped"])


def fold(sums, sumsq, k, X, n_samples):
    """lightmap_common.fold's rule on X, and Q[k] += l(X) * l(X) beside it (sumsq None: the sums alone); s ascending"""
    x4 = np.concatenate([X, np.zeros((len(X), 1), F)], 1)
    out = LC.fold(sums, k, x4, n_samples)
    if sumsq is None:
        return out, None
    q = np.array(sumsq, F).reshape(-1)
    l = lum(np.asarray(X, F)).reshape(len(k), n_samples)
    for s in range(n_samples):
        q[k] = q[k] + l[:, s] * l[:, s]
    assert q.dtype == F
    return out, q.reshape(np.shape(sumsq))


# ---- the scenes
def _quad_at(lo, hi, z, down=True):
    """an axis-aligned quad [lo, hi] at height z, two triangles, facing -z (down) or +z"""
    (x0, y0), (x1, y1) = lo, hi
    p = np.array([[[x0, y0, z], [x1, y0, z], [x1, y1, z]], [[x0, y0, z], [x1, y1, z], [x0, y1, z]]], F)
    n = np.tile(np.array([0, 0, -1 if down else 1], F), (2, 3, 1))
    return p, n


def blocker_model():
    from path_tracer_amd.scene_desc import Lambertian, Model
    p, n = _quad_at((0.1, 0.1), (0.55, 0.6), 0.8)
    return Model.new(p, n, Lambertian.new((0.6, 0.5, 0.4)), None, "blocker")


def two_lamp_scene():
    """lightmap_common's unit quad under two lamps of unequal area and colour (two emissive MODELS: the CDF spans both) and a small blocker"""
    from path_tracer_amd.scene_desc import Emissive, Lambertian, Model, SceneDesc
    floor = Model.new(LC.QUAD_POS, LC.QUAD_NRM, Lambertian.new((0.8, 0.8, 0.8)), None, "quad", uvs=LC.QUAD_UV)
    ap, an = _quad_at((0.0, 0.0), (1.0, 1.0), 2.0)
    bp, bn = _quad_at((0.9, 0.2), (1.4, 0.7), 1.5)
    return SceneDesc.new([floor, Model.new(ap, an, Emissive.new((5.0, 5.0, 5.0)), None, "lamp_a"), blocker_model(),
                          Model.new(bp, bn, Emissive.new((2.0, 6.0, 3.0)), None, "lamp_b")], None, "two lamps")


def emission_textured_scene():
    """the unit quad under one lamp whose UVs vary across its triangles (beyond [0, 1), negative) on a 5 x 3 emission texture of random
    texels, and the blocker"""
    from path_tracer_amd.scene_desc import Emissive, Lambertian, Model, SceneDesc, Texture
    rng = np.random.default_rng(11)
    tex = Texture.new(rng.uniform(0.5, 6.0, (3, 5, 3)).astype(F))
    lamp = Emissive.new((1.0, 0.8, 0.6)).emission_textured(tex)
    floor = Model.new(LC.QUAD_POS, LC.QUAD_NRM, Lambertian.new((0.8, 0.8, 0.8)), None, "quad", uvs=LC.QUAD_UV)
    lp, ln = _quad_at((-0.25, -0.25), (1.25, 1.25), 2.0)
    l_uv = np.array([[[-1.25, 0.1], [0.7, -0.4], [1.9, 1.3]], [[-1.25, 0.1], [1.9, 1.3], [-0.3, 2.2]]], F)
    return SceneDesc.new([floor, Model.new(lp, ln, lamp, None, "lamp", uvs=l_uv), blocker_model()], None, "emission-textured lamp")


def moved_instanced_scene(w=48, h=32):
    """scenes.cornell_instanced under the box atlas with its general-rigid instance moved (lightmap_common.moved_matrices)"""
    sc = LC.instanced_atlas_scene(w, h)
    sc.models[LC.INSTANCED_MODEL].matrices = LC.moved_matrices(sc)
    return sc


CASES = ("quad", "short", "two_lamps", "emtex", "instanced")
_SCENES = {}


def case(name):
    """(scene, model, instance, w, h, max_bounces, enable_nee) of a named case.  The oracle knows no textures, so the emission-textured case
    gathers at max_bounces = 0 with NEE off: a gather ray then returns the ambient term on a miss, nothing on a surface, and on the lamp the
    emission that X zeroes - none of which reads the texture - while every D does"""
    if name not in _SCENES:
        if name == "quad":
            _SCENES[name] = (LC.quad_scene(light=True), 0, 0, 8, 8, DEPTH, 1)
        elif name == "short":
            sc, model = LC.cornell_atlas_scene("cb_box_short")
            _SCENES[name] = (sc, model, 0, 12, 8, DEPTH, 1)
        elif name == "two_lamps":
            _SCENES[name] = (two_lamp_scene(), 0, 0, 8, 8, DEPTH, 1)
        elif name == "emtex":
            _SCENES[name] = (emission_textured_scene(), 0, 0, 8, 8, 0, 0)
        elif name == "instanced":
            _SCENES[name] = (moved_instanced_scene(), LC.INSTANCED_MODEL, LC.INSTANCED_INSTANCE, 12, 8, DEPTH, 1)
    return _SCENES[name]


_ORACLES = {}


def oracle_of(O, name):
    if name not in _ORACLES:
        _ORACLES[name] = O.Oracle(case(name)[0])
    return _ORACLES[name]


def table_of(name):
    sc, model, instance, w, h = case(name)[:5]
    m = sc.models[model]
    return LC.texels(m.positions, m.normals, m.uvs, m.matrices[instance], w, h)


_HOOK = {}


def hook_inputs(O, name, n_samples=8, light_key_base=5000, bias=0.25):
    """(keys, samples, o, n, the restated light samples) of every (covered texel, sample) of a case: what the hook tests compare"""
    if name not in _HOOK:
        table = table_of(name)
        prim, _, position, normal = table
        k = np.flatnonzero(prim.reshape(-1) != LC.MISS)
        n = np.repeat(normal.reshape(-1, 3)[k], n_samples, 0)
        o = np.repeat((position.reshape(-1, 3)[k] + F(bias) * normal.reshape(-1, 3)[k]).astype(F), n_samples, 0)
        keys = np.repeat((k + light_key_base).astype(np.uint32), n_samples)
        smp = np.tile(np.arange(n_samples, dtype=np.uint32), len(k))
        orc = oracle_of(O, name)
        ls = light_samples(LightTable(orc, case(name)[0]), keys, smp, o, n)
        ls["blocked"] = shadowed(orc, o, ls)
        _HOOK[name] = (keys, smp, o, n, ls)
    return _HOOK[name]


_BAKES = {}


def expected_bake(O, name, n_samples, first_sample=0, key_base=0, bias=0.25):
    """bake_samples of a case, computed once"""
    key = (name, n_samples, first_sample, key_base, bias)
    if key not in _BAKES:
        sc, _, _, _, _, depth, nee = case(name)
        _BAKES[key] = bake_samples(O, oracle_of(O, name), sc, table_of(name), n_samples, first_sample, key_base, None, bias, depth, nee)
    return _BAKES[key]


def renderer(api, name, flags=0, **kw):
    sc, _, _, _, _, depth, nee = case(name)
    return api.Renderer(sc, 48, 32, max_bounces=depth, enable_nee=bool(nee), flags=flags, **kw)


# ---- Lambert's closed form for the irradiance of a polygon
def polygon_irradiance(p, n, vertices, radiance):
    """E = Le / 2 * |sum over edges of gamma_e * (n . Gamma_e)| at point p with unit normal n, of the polygon `vertices` [m, 3] wholly above
    p's horizon; binary64.  gamma_e: the angle the edge subtends at p; Gamma_e: the unit normal of the plane through p and the edge"""
    v = np.asarray(vertices, D64) - np.asarray(p, D64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    total = 0.0
    for a, b in zip(v, np.roll(v, -1, 0)):
        gamma = np.arccos(np.clip(a @ b, -1.0, 1.0))
        cr = np.cross(a, b)
        total += gamma * (np.asarray(n, D64) @ (cr / np.linalg.norm(cr)))
    return radiance * abs(total) / 2.0
