"""Shared by tests/test_normalmap_host.py and tests/test_gpu_normalmap.py: the definition of the normal-mapped shading normal (include/pt_api.h)
restated in numpy, every product, sum, difference and quotient ONE np.float32 operation in the order the header writes them, and the scenes the
tests use.  Nothing here calls the library."""
import numpy as np

from path_tracer_amd.scene_desc import GGX, IDENTITY_3x4, Camera, Emissive, Lambertian, Model, SceneDesc, Specular, Texture
from textures_common import F, as_u32, bilinear, box, quad, world_instance_models

FLAT = (0.5, 0.5, 1.0)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def unit3(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt(dot(a, a))[..., None]


def tangents(positions, uvs):
    """positions [n, 3, 3], uvs [n, 3, 2] (load order) -> T [n, 3], sign [n]; (0, 0, 0), +1 where det == 0 or T is not finite"""
    p = np.asarray(positions, F); uv = np.asarray(uvs, F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        d1, d2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
        t = (e1 * d2[:, 1, None] - e2 * d1[:, 1, None]) / det[:, None]
        b = (e2 * d1[:, 0, None] - e1 * d2[:, 0, None]) / det[:, None]
        sign = np.where(dot(cross(e1, e2), cross(t, b)) < F(0.0), F(-1.0), F(1.0)).astype(F)
    none = (det == F(0.0)) | ~np.isfinite(t).all(axis=1)
    t[none] = F(0.0)
    sign[none] = F(1.0)
    return t.astype(F), sign


def bilinear_const(tex, s, t):
    """the normal map's lookup: textures_common.bilinear, except that four equal texels are that texel, with no arithmetic"""
    tex = np.asarray(tex, F)
    h, w = tex.shape[0], tex.shape[1]
    out = bilinear(tex, s, t)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, y0 = as_u32(F(w) * np.asarray(s, F)), as_u32(F(h) * np.asarray(t, F))
    one64, m32 = np.uint64(1), np.uint64(0xFFFFFFFF)
    xa, xb = x0 % np.uint64(w), ((x0 + one64) & m32) % np.uint64(w)
    ya, yb = y0 % np.uint64(h), ((y0 + one64) & m32) % np.uint64(h)
    c00, c01, c10, c11 = tex[ya, xa], tex[yb, xa], tex[ya, xb], tex[yb, xb]
    same = ((c00 == c01) & (c00 == c10) & (c00 == c11)).all(axis=-1)
    out[same] = c00[same]
    return out


def perturbed_normal(n, tex, uv3, tan, sign, u, v):
    """object-space N' of hits: n [k, 3] the unit interpolated normals, tex [h, w, 3] or None, uv3 [k, 3, 2], tan [k, 3], sign [k]"""
    if tex is None:
        return n.copy()
    u = np.asarray(u, F); v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        st = []
        for k in (0, 1):
            a, b, c = uv3[:, 0, k], uv3[:, 1, k], uv3[:, 2, k]
            x = (a + u * (b - a)) + v * (c - a)
            st.append(x - np.floor(x))
        c = bilinear_const(tex, st[0], st[1])
        xyz = F(2.0) * c - F(1.0)
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        keep = ((x == F(0.0)) & (y == F(0.0))) | (tan == F(0.0)).all(axis=1)
        tp = unit3(tan - n * dot(n, tan)[:, None])
        bp = cross(n, tp) * sign[:, None]
        out = unit3((tp * x[:, None] + bp * y[:, None]) + n * z[:, None])
    out[keep] = n[keep]
    return out.astype(F)


def rows3(m, x):
    """(r0 . x, r1 . x, r2 . x) of the 3x3 of m [k, 3, 4], each dot (a + b) + c"""
    return np.stack([(m[:, r, 0] * x[:, 0] + m[:, r, 1] * x[:, 1]) + m[:, r, 2] * x[:, 2] for r in range(3)], axis=-1)


def scene_shading_normal(desc, matrix, inv_matrix, instance, prim, u, v, direction):
    """the restated world shading normal [k, 3] and front flag [k] of hits on a scene description; matrix / inv_matrix: the world TLAS's
    instance matrices [n_inst, 3, 4] (Renderer.tlas_instances(0): inputs of the definition)"""
    instance = np.asarray(instance); prim = np.asarray(prim)
    u = np.asarray(u, F); v = np.asarray(v, F); d = np.asarray(direction, F)
    out = np.zeros((len(instance), 3), F)
    front = np.zeros(len(instance), np.uint8)
    models = world_instance_models(desc)[instance]
    for mi in np.unique(models):
        sel = np.nonzero(models == mi)[0]
        mod = desc.models[int(mi)]
        pr = prim[sel]
        nv = np.asarray(mod.normals, F)[pr]
        uu, vv = u[sel], v[sel]
        wgt = F(1.0) - uu - vv
        n = unit3((nv[:, 0] * wgt[:, None] + nv[:, 1] * uu[:, None]) + nv[:, 2] * vv[:, None])
        inv, fwd = inv_matrix[instance[sel]], matrix[instance[sel]]
        fr = dot(rows3(inv, d[sel]), n) < F(0.0)
        tex = mod.material.normal_texture
        if mod.uvs is None:
            uv = np.zeros((mod.positions.shape[0], 3, 2), F)
            tan, sign = np.zeros((mod.positions.shape[0], 3), F), np.ones(mod.positions.shape[0], F)
        else:
            uv = np.asarray(mod.uvs, F)
            tan, sign = tangents(mod.positions, uv)
        m = perturbed_normal(n, None if tex is None else tex.data, uv[pr], tan[pr], sign[pr], uu, vv)
        m = np.where(fr[:, None], m, -m)
        out[sel] = rows3(fwd, m)
        front[sel] = fr
    return out, front


def encode(v):
    """a tangent-space vector (or array of them) as texels: 0.5 * v + 0.5"""
    return (F(0.5) * np.asarray(v, F) + F(0.5)).astype(F)


def bumpy_texture(w, h, seed, amount=0.6):
    """w x h texels of distinct, non-flat unit vectors with z > 0"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-amount, amount, (h, w, 2))
    xy[np.abs(xy) < 0.05] = 0.1
    z = np.sqrt(1.0 - (xy ** 2).sum(axis=2))
    return Texture.new(encode(np.concatenate([xy, z[..., None]], axis=2)))


def flat_texture(w, h):
    return Texture.new(np.broadcast_to(np.array(FLAT, F), (h, w, 3)).copy())


# ---------------------------------------------------------------------------------------------------------------------------------- scenes
def general_turn(seed=3):
    """a rotation about a general axis whose binary32 columns pass Model::new's rigidity check (exact unit lengths): the first of a seeded search"""
    from path_tracer_amd.scene_desc import is_rigid
    rng = np.random.default_rng(seed)
    for _ in range(100000):
        a = rng.normal(size=3); a = a / np.sqrt((a * a).sum())
        ang = rng.uniform(0.4, 2.6)
        c, s = np.cos(ang), np.sin(ang)
        k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        m = np.zeros((3, 4), F)
        m[:, :3] = (np.eye(3) + s * k + (1 - c) * (k @ k)).astype(F)
        if is_rigid(m) and np.abs(m[:, :3]).min() > 0.05:
            return m
    raise AssertionError("no rigid turn found")


def hook_scene(flat=False):
    """the unit hook's scene: a box with interpolated (non-flat) vertex normals under a 5 x 3 map, placed twice (identity and a general rigid
    turn), with mirrored, degenerate, negative, exactly-1 and 1e6 UVs; a quad WITHOUT UVs under a 1 x 1 map; a box under an 8 x 4 map that is
    also colour-textured; an unmapped quad; a light.  flat: every map is all (0.5, 0.5, 1.0)"""
    rng = np.random.default_rng(11)
    t53 = flat_texture(5, 3) if flat else bumpy_texture(5, 3, 1)
    t11 = flat_texture(1, 1) if flat else Texture.new(encode([[[0.3, -0.4, np.sqrt(0.75)]]]))
    t84 = flat_texture(8, 4) if flat else bumpy_texture(8, 4, 2)
    colour = Texture.new(rng.uniform(0.1, 0.9, (2, 2, 3)).astype(F))
    bp, bn = box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    # interpolated normals: every vertex normal leans towards its corner
    lean = (bn.astype(np.float64) + 0.35 * bp / np.sqrt(3.0))
    bn2 = (lean / np.sqrt((lean ** 2).sum(axis=2, keepdims=True))).astype(F)
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
        Model.new(bp, bn2, Lambertian.new((0.8, 0.6, 0.4)).normal_mapped(t53), two, "instanced", uvs=uv),
        Model.new(qp, qn, GGX.new_metal((1.0, 1.0, 1.0), 0.4).normal_mapped(t11), None, "no uvs"),
        Model.new(lp, ln, Emissive.new((5.0, 5.0, 5.0)), None, "light"),
        Model.new(bp + F(20.0), bn, Lambertian.new((0.3, 0.9, 0.5)).textured(colour).normal_mapped(t84), None, "eight by four",
                  uvs=rng.uniform(0.0, 1.0, (12, 3, 2)).astype(F)),
        Model.new(qp + F(0.5), qn, Lambertian.new((0.1, 0.2, 0.3)), None, "unmapped", uvs=rng.uniform(0.0, 1.0, (2, 3, 2)).astype(F)),
    ]
    return SceneDesc.new(models, None, "shading normal")


def hook_queries(desc, n=3000):
    rng = np.random.default_rng(8)
    inst_model = world_instance_models(desc)
    inst = rng.integers(0, len(inst_model), n).astype(np.uint32)
    ntri = np.array([desc.models[m].positions.shape[0] for m in inst_model])[inst]
    prim = (rng.integers(0, 1 << 30, n) % ntri).astype(np.uint32)
    u = rng.uniform(0.0, 1.0, n).astype(F)
    v = (rng.uniform(0.0, 1.0, n).astype(F) * (F(1.0) - u)).astype(F)
    u[:6] = [0.0, 1.0, 0.0, 0.5, 0.25, 1.0]; v[:6] = [0.0, 0.0, 1.0, 0.5, 0.75, 0.0]   # the vertices and an edge
    # every special triangle of the instanced model is asked about, through both instances
    inst[6:20] = [0, 1] * 7; prim[6:20] = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    d = rng.normal(size=(n, 3))                                                        # any direction: front and back faces alike
    d = (d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(F)
    return inst, prim, u, v, d


def quad_scene(width, height, material, light=True, seed=4):
    """ONE quad (two triangles) with UVs that vary across it (beyond [0, 1), negative, the second triangle's winding mirrored in UV space) under a
    5 x 3 normal map of distinct, non-flat texels; a small light above it when asked for.  The quad is model 0 (identity instance)."""
    tex = bumpy_texture(5, 3, seed, amount=0.45)
    fp, fn = quad((-8.0, -4.0, -8.0), (-8.0, -4.0, 8.0), (8.0, -4.0, 8.0), (8.0, -4.0, -8.0))
    f_uv = np.array([[[0.0, 0.0], [0.0, 2.75], [3.5, 2.75]], [[-1.25, 0.1], [1.9, 1.3], [-0.3, 2.2]]], F)
    models = [Model.new(fp, fn, material.normal_mapped(tex), None, "quad", uvs=f_uv)]
    if light:
        lp, ln = quad((-1.0, 5.0, -1.0), (1.0, 5.0, -1.0), (1.0, 5.0, 1.0), (-1.0, 5.0, 1.0))
        models.append(Model.new(lp, ln, Emissive.new((30.0, 25.0, 20.0)), None, "light"))
    return SceneDesc.new(models, Camera.new((1.0, 3.0, 9.0), (0.0, -4.0, -1.0), 60.0, width / height), "normal-mapped quad")


TILT = (0.35, -0.25)


def tilt_scene(width, height, how):
    """a Lambertian floor under a small area light.  how = 'map': the floor's whole normal map is ONE tilted texel; 'flat': the flat map;
    'vertex' (needs normals=...): no map, the vertex normals given"""
    fp, fn = quad((-8.0, -4.0, -8.0), (-8.0, -4.0, 8.0), (8.0, -4.0, 8.0), (8.0, -4.0, -8.0))
    f_uv = np.array([[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]], F)
    x, y = TILT
    tilted = Texture.new(encode([[[x, y, np.sqrt(1.0 - x * x - y * y)]]]))
    lam = Lambertian.new((0.8, 0.7, 0.6))
    lp, ln = quad((-1.5, 3.0, -1.5), (1.5, 3.0, -1.5), (1.5, 3.0, 1.5), (-1.5, 3.0, 1.5))
    light = Model.new(lp, ln, Emissive.new((20.0, 18.0, 15.0)), None, "light")
    cam = Camera.new((0.0, 4.0, 10.0), (0.0, -4.0, 0.0), 55.0, width / height)
    if isinstance(how, str) and how == "map":
        floor = Model.new(fp, fn, lam.normal_mapped(tilted), None, "floor", uvs=f_uv)
    elif isinstance(how, str) and how == "flat":
        floor = Model.new(fp, fn, lam.normal_mapped(flat_texture(1, 1)), None, "floor", uvs=f_uv)
    else:
        floor = Model.new(fp, np.broadcast_to(np.asarray(how, F), fp.shape).copy(), lam, None, "floor")
    return SceneDesc.new([floor, light], cam, "tilted floor")


def tilt_normal():
    """the restated object-space N' of the tilted map on the floor (one value: the floor is flat, its UV frame the same on both triangles)"""
    desc = tilt_scene(16, 16, "map")
    fl = desc.models[0]
    tan, sign = tangents(fl.positions, fl.uvs)
    n = np.asarray(fl.normals, F)[:, 0]
    out = perturbed_normal(n, fl.material.normal_texture.data, np.asarray(fl.uvs, F), tan, sign, np.array([0.25, 0.25], F), np.array([0.25, 0.25], F))
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    return out[0]


# ---------------------------------------------------------------------------------------------------------------------------------- composition
M64 = (1 << 64) - 1
SEED = 0x5EED5EED
EPSILON = F(5e-04)


def stream_f32(pixel, sample, k, seed=SEED):
    """draw k (0 = the camera's) of the stream of (pixel, sample): stream_key + the k-th WyRand output, (u32 as f32) / 2^32  (pt_math.h)"""
    z = (seed + 0x9E3779B97F4A7C15 * ((int(sample) << 32) | int(pixel))) & M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    st = (z + (k + 1) * 0xA0761D6478BD642F) & M64
    m = st ^ 0xE7037ED1A0B428DB
    v = (((st * m) >> 64) ^ ((st * m) & M64)) & 0xFFFFFFFF
    return F(np.uint32(v)) / F(4294967296.0)


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


def _mis2(f, g):
    return (f * f) / (f * f + g * g)


def direct_light(orc, light, p, s, d, at, nrm, front):
    """both direct-light estimates (integrator.rs:25-130) of a hit of the oracle's material 0 at `at` with shading normal nrm, from oracle
    pieces: the light sampler's table, pt_bsdf_eval at the sampled light direction, pt_material_eval for the BSDF-sampled direction, the
    oracle's any-hit and lights-TLAS traces.  light: the scene's one emissive model (lights BLAS 0).  The stream stands at draw 1.
    Returns (explicit, bsdf-sampled, draws consumed)"""
    emitted = np.array(light.material.colour, F)
    cdf = orc.light_cdf()
    zero = np.zeros(3, F)

    def area(prim):
        n0 = orc.triangle(0, int(prim), which=1)[0:3]
        return F(0.5) * np.sqrt(dot(n0, n0))

    # ---- estimate_direct_explicit: x, lu, lv
    x = stream_f32(p, s, 1)
    li = min(int((cdf["cdf"] < x).sum()), len(cdf["cdf"]) - 1)
    lu, lv = stream_f32(p, s, 2), stream_f32(p, s, 3)
    if lu + lv > F(1.0):
        lu, lv = F(1.0) - lu, F(1.0) - lv
    lw = F(1.0) - lu - lv
    prim = int(cdf["prim"][li])
    P, N = np.asarray(light.positions, F)[prim], np.asarray(light.normals, F)[prim]
    point = (P[0] * lw + P[1] * lu) + P[2] * lv
    lnormal = unit3((N[0] * lw + N[1] * lu) + N[2] * lv)
    dd = point - at
    dist2 = dot(dd, dd)
    dist = np.sqrt(dist2)
    dr = unit3(dd)
    e = zero
    if dot(dr, nrm) > F(0.0) and not orc.trace_any(at[None], dr[None], [(F(1.0) - EPSILON) * dist])[0]:
        bp = orc.bsdf_eval(0, d[None], dr[None], nrm[None], [front])[0]
        sample_pdf = cdf["pdf"][li] / area(prim)
        cosine = np.abs(dot(dr, lnormal))
        light_pdf = sample_pdf * (dist2 / cosine)
        e = emitted * _mis2(light_pdf, bp[3]) * np.abs(dot(dr, nrm)) * bp[0:3] / light_pdf
    # ---- estimate_direct_bsdf
    ev = orc.material_eval(0, d, nrm, front, p, s, draws_consumed=4)
    wo, bsdf, pdf, weak, draws = ev[0:3], ev[3:6], ev[6], ev[7], int(ev[8])
    b = zero
    if dot(wo, nrm) > F(0.0):
        lh = orc.trace_closest(at[None], wo[None], which=1)
        if lh["inst"][0] != 0xFFFFFFFF and not orc.trace_any(at[None], wo[None], [lh["t"][0] * (F(1.0) - EPSILON)])[0] and pdf > F(0.0):
            a = area(lh["prim"][0])
            sample_pdf = (a * np.sqrt(dot(emitted, emitted)) / F(cdf["max"])) / a
            cosine = np.abs(dot(wo, lh["normal"][0]))
            light_pdf = sample_pdf * (lh["t"][0] * lh["t"][0] / cosine)
            b = emitted * _mis2(pdf, light_pdf) * weak * bsdf / pdf
    return e.astype(F), b.astype(F), 3 + draws


def composed_sample(orc, desc, light, o, d, p, s, h, nrm, front, nee):
    """one sample of a camera ray that hit the quad (material 0 of the oracle's scene) at max_bounces = 1, with nrm as the shading normal.
    The direct light of the hit (NEE on, a material that is not a delta), then ONE bounce whose direction, bsdf, pdf and weakening are
    pt_material_eval's: a miss adds 0.006 * pw; a light adds emitted * pw only without NEE or after a delta bounce; the quad again is
    refused (it cannot be seen from itself)"""
    delta = desc.models[0].material.kind in (2, 5)
    emitted = np.array(light.material.colour, F)
    at = np.array([fma32(d[k], h["t"][0], o[k]) for k in range(3)], F)                      # r.at(t): mul_add per component
    acc = np.zeros(3, F)
    draws = 1
    if nee and not delta:
        e, b, used = direct_light(orc, light, p, s, d, at, nrm, front)
        acc = acc + np.ones(3, F) * (e + b)
        draws += used
    ev = orc.material_eval(0, d, nrm, front, p, s, draws_consumed=draws)                   # wo xyz, bsdf rgb, pdf, weakening, draws
    wo, bsdf, pdf, weak = ev[0:3], ev[3:6], ev[6], ev[7]
    if not pdf < F(0.0):                                                                   # MIN_PDF = 0
        with np.errstate(invalid="ignore", divide="ignore"):
            pw = (weak * bsdf) / pdf
        h2 = orc.trace_closest(at[None], wo[None])
        if h2["inst"][0] == 0xFFFFFFFF:
            acc = acc + F(0.006) * pw
        else:
            assert world_instance_models(desc)[h2["inst"][0]] == 1, "the bounce sees the light or nothing"
            if not nee or delta:
                acc = np.array([fma32(emitted[k], pw[k], acc[k]) for k in range(3)], F)
    if not np.isfinite(acc).all():                                                         # integrator.rs:272
        acc = np.zeros(3, F)
    assert float(np.sqrt((acc.astype(np.float64) ** 2).sum())) < 99.0                     # below the 100 clamp: it never has to be restated
    return np.array([acc[0], acc[1], acc[2], 1.0], F)


def composed_samples(oracle_mod, desc, matrix, inv_matrix, w, h, spp, nee, mapped=True):
    """every sample of quad_scene's description at max_bounces = 1: hits on the quad composed (composed_sample) with the restated N' as the
    shading normal (mapped=False: with the oracle's own normal, which must then reproduce the oracle's integrate()), everything else the
    oracle's integrate().  Returns (samples [spp, h, w, 4], hits on the quad, hits whose normal the map moved)"""
    import dataclasses
    plain = dataclasses.replace(desc.models[0], material=desc.models[0].material.normal_mapped(None), uvs=None)
    orc = oracle_mod.Oracle(SceneDesc.new([plain] + list(desc.models[1:]), desc.camera))
    inst_model = world_instance_models(desc)
    want = np.zeros((spp, h, w, 4), F)
    n_quad = n_moved = 0
    for s in range(spp):
        for p in range(w * h):
            o, d = orc.primary_ray(w, h, p, s)
            hit = orc.trace_closest(o[None], d[None])
            mi = int(inst_model[hit["inst"][0]]) if hit["inst"][0] != 0xFFFFFFFF else -1
            if mi != 0:
                want[s, p // w, p % w] = orc.integrate(o, d, p, s, 1, max_bounces=1, enable_nee=int(nee))[0]
                continue
            n_quad += 1
            nrm, front = hit["normal"][0], int(hit["front"][0])
            if mapped:
                nn, ff = scene_shading_normal(desc, matrix, inv_matrix, hit["inst"], hit["prim"], hit["u"], hit["v"], d[None])
                assert int(ff[0]) == front
                n_moved += int(not np.array_equal(nn[0], nrm))
                nrm = nn[0]
            want[s, p // w, p % w] = composed_sample(orc, desc, desc.models[1], o, d, p, s, hit, nrm, front, nee)
    return want, n_quad, n_moved
