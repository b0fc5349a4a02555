"""Shared by tests/test_guides_follow_host.py and tests/test_gpu_guides_follow.py: the definition of the followed guides (include/pt_api.h,
pt_render_guides_followed) restated in numpy, every product, sum and difference ONE np.float32 operation in the order the header writes
them, over the oracle's trace_closest; and the room the tests render.  Nothing here calls the library's device code."""
import numpy as np

from path_tracer_amd import scenes
from path_tracer_amd.scene_desc import (DIELECTRIC, SPECULAR, Camera, Dielectric, Emissive, GGX, Lambertian, Model, SceneDesc, Specular,
                                        Texture)
from textures_common import const_uvs, scene_surface_colour, world_instance_models

F = np.float32
MISS = 0xFFFFFFFF
W, H = 48, 32
MAX_HOPS = 8


# ---------------------------------------------------------------------------------------------------------------------------- arithmetic
def fma32(a, b, c):
    """f32::mul_add per element: a * b + c rounded ONCE to binary32.  The product of two binary32 values is exact in binary64; the sum is
    rounded to odd there (TwoSum gives the residual), which makes the final rounding to binary32 the correct one"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0.0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]                                    # glam dot3


def reflect(i, n):
    """utility.rs:21: i - 2 * dot(n, i) * n"""
    return i - (F(2.0) * dot(n, i))[:, None] * n


def refract(i, n, eta):
    """utility.rs:23-36; NaN in every component where k <= 0 (total internal reflection)"""
    with np.errstate(invalid="ignore"):
        ndi = dot(n, i)
        k = F(1.0) - eta * eta * (F(1.0) - ndi * ndi)
        out = eta[:, None] * i - (eta * ndi + np.sqrt(k))[:, None] * n
    out[k <= F(0.0)] = np.nan
    return out


def follow_dir(kind, ior, d, n, front):
    """the follow-on direction of the definition at hits of ONE material: (wo [m, 3], followed [m], total internal reflection [m])"""
    d = np.asarray(d, F).reshape(-1, 3); n = np.asarray(n, F).reshape(-1, 3)
    m = d.shape[0]
    if kind == SPECULAR:
        return reflect(d, n), np.ones(m, bool), np.zeros(m, bool)
    if kind == DIELECTRIC:
        eta = np.where(np.asarray(front).astype(bool), F(1.0) / F(ior), F(ior)).astype(F)
        r = refract(d, n, eta)
        tir = np.isnan(r).any(axis=1)
        r[tir] = reflect(d[tir], n[tir])
        return r, np.ones(m, bool), tir
    return np.zeros((m, 3), F), np.zeros(m, bool), np.zeros(m, bool)


# ------------------------------------------------------------------------------------------------------------------------------ the chain
def chains(orc, desc, o, d, max_hops):
    """the six guides of rays (o, d) [n, 3] followed through `desc` (the oracle `orc` holds the same scene), and what the chains met:
    position [n, 4], normal [n, 3], model [n], instance [n], albedo [n, 3], hops [n]; tir [n]: some hop was a total internal reflection;
    hop_model [n, max_hops + 1] (the model hit at every hop, -1 beyond the chain's end) and hop_front likewise; dirs and hop_normal [n, max_hops + 1, 3]: every hop's ray direction and face-forwarded normal"""
    o = np.asarray(o, F).reshape(-1, 3).copy(); d = np.asarray(d, F).reshape(-1, 3).copy()
    n = o.shape[0]
    leaf_model = world_instance_models(desc)
    out = dict(position=np.zeros((n, 4), F), normal=np.zeros((n, 3), F), model=np.zeros(n, np.uint32), instance=np.zeros(n, np.uint32),
               albedo=np.zeros((n, 3), F), hops=np.zeros(n, np.uint8), tir=np.zeros(n, bool), hop_model=np.full((n, max_hops + 1), -1, np.int64),
               hop_front=np.full((n, max_hops + 1), -1, np.int64), dirs=np.zeros((n, max_hops + 1, 3), F),
               hop_normal=np.zeros((n, max_hops + 1, 3), F))
    live = np.arange(n)
    prod = tsum = None
    for h in range(max_hops + 1):
        if live.size == 0:
            break
        out["dirs"][live, h] = d
        tc = orc.trace_closest(o, d)
        hit = tc["inst"] != MISS
        miss = live[~hit]
        far = fma32(d[~hit], F(1e5), o[~hit])
        out["position"][miss] = np.concatenate([far, np.full((len(miss), 1), 1e5, F)], axis=1)
        out["model"][miss] = MISS; out["instance"][miss] = MISS
        out["hops"][miss] = h                                                     # (normal and albedo stay 0)
        live, o, d = live[hit], o[hit], d[hit]
        if prod is not None:
            prod, tsum = prod[hit], tsum[hit]
        inst, t = tc["inst"][hit], tc["t"][hit]
        nrm, front = tc["normal"][hit], tc["front"][hit]
        p = fma32(d, t[:, None], o)
        c = scene_surface_colour(desc, leaf_model, inst, tc["prim"][hit], tc["u"][hit], tc["v"][hit])
        if h:
            c = prod * c
            t = tsum + t
        model = leaf_model[inst]
        out["hop_model"][live, h] = model; out["hop_front"][live, h] = front; out["hop_normal"][live, h] = nrm
        wo = np.zeros_like(d); go = np.zeros(len(live), bool)
        for mi in np.unique(model):
            sel = model == mi
            mat = desc.models[int(mi)].material
            w, followed, tir = follow_dir(mat.kind, mat.ior, d[sel], nrm[sel], front[sel])
            wo[sel] = w; go[sel] = followed & (h < max_hops)
            out["tir"][live[sel]] |= tir & go[sel]
        end = live[~go]
        out["position"][end] = np.concatenate([p[~go], t[~go, None]], axis=1)
        out["normal"][end] = nrm[~go]
        out["model"][end] = model[~go].astype(np.uint32) | np.uint32(h << 28)
        out["instance"][end] = inst[~go]
        out["albedo"][end] = c[~go]
        out["hops"][end] = h
        live, o, d, prod, tsum = live[go], p[go], wo[go], c[go], t[go]
    return out


def pinhole_rays(orc, w, h, sample, pixels=None):
    """the oracle's camera rays of `sample` of the given global pixels (all of them: row-major)"""
    pixels = range(w * h) if pixels is None else pixels
    rays = [orc.primary_ray(w, h, int(p), sample) for p in pixels]
    return np.array([r[0] for r in rays], F), np.array([r[1] for r in rays], F)


def library_rays(r, w, rows, sample):
    """pt_primary_ray's camera rays (host evaluation; tests/test_lens_host.py and tests/test_projection_host.py hold it to the definitions)
    of `sample` of the pixels of the given global rows, under the lens or projection in force"""
    rays = [r.primary_ray(int(gy) * w + x, sample)[:2] for gy in rows for x in range(w)]
    return np.array([q[0] for q in rays], F), np.array([q[1] for q in rays], F)


def shaped(g, rows, w):
    """a chains() result as the library's read-backs shape it: [rows, w, ..]"""
    return {k: v.reshape((rows, w) + v.shape[1:]) for k, v in g.items()}


# -------------------------------------------------------------------------------------------------------------------------------- the room
def _quad(a, b, c, d):
    p = np.array([[a, b, c], [a, c, d]], np.float64)
    n = np.cross(p[0, 1] - p[0, 0], p[0, 2] - p[0, 0])
    n = n / np.sqrt((n * n).sum())
    return p, np.broadcast_to(n, p.shape).copy()


def _solid(faces):
    """triangles with flat normals as wound (counter-clockwise seen from outside)"""
    ps, ns = [], []
    for f in faces:
        if len(f) == 4:
            p, n = _quad(*f)
        else:
            p = np.array([f], np.float64)
            n = np.cross(p[0, 1] - p[0, 0], p[0, 2] - p[0, 0]); n = np.broadcast_to(n / np.sqrt((n * n).sum()), p.shape).copy()
        ps.append(p); ns.append(n)
    return np.concatenate(ps), np.concatenate(ns)


def _box(lo, hi):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    return _solid([((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)), ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)),
                   ((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), ((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),
                   ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0))])


def _placed(tris, normals, material, quat, name, uvs=None):
    """a model whose WORLD geometry is (tris, normals), held in object space under a general rigid instance matrix built glam's way from the
    quaternion (scenes.rigid_from_quat): the vertices are taken back through the matrix in binary64 and rounded once, so the instance
    transform, its inverse and the normal transform all carry inexact entries"""
    m = scenes.rigid_from_quat(*quat, translation=(3.0, -2.0, 1.0))
    rot, tr = m[:, :3].astype(np.float64), m[:, 3].astype(np.float64)
    inv = np.linalg.inv(rot)
    local = (tris - tr) @ inv.T
    return Model.new(local.astype(F), (normals @ inv.T).astype(F), material, m[None], name, uvs=uvs)


ROOM_MODELS = ["light", "back", "wall_a", "wall_b", "mirror", "slab", "prism", "lower", "upper", "floor"]
LOUD = 50.0


def follow_room(w=W, h=H, camera=None):
    """An open room for the guide chains, seen from (0, 0, 12) towards -z:
      mirror       a flat tinted mirror at z = -12 that shows the two textured walls behind the camera (z = 20) and the boundary between them
      wall_a / _b  Lambertian on ONE 2 x 2 texture, every vertex of a model at one texel corner (the other texels are LOUD), split at x = -10
      slab         a glass pane, two parallel faces at z = 3 and z = 2: chains enter, leave through the back face, and end on the back wall
      prism        a right-angled glass prism below the eye line: rays enter its front face and meet the hypotenuse beyond the critical angle
      lower/upper  two mirrors facing each other, a wedge one unit high at its mouth that narrows over 20 units: every bounce off the upper one
                   steepens the ray until it turns round, so chains run into the hop cap; the upper one's other side faces the open sky
                   (and the light): chains that end as a miss after one hop
      back, floor  plain Lambertian; light: an emissive quad overhead
    Every model but the light stands under a general rigid instance matrix."""
    tex = np.full((2, 2, 3), LOUD, F)
    tex[0, 0] = (0.8, 0.3, 0.2); tex[0, 1] = (0.2, 0.4, 0.9)
    texture = Texture.new(tex)
    wall = Lambertian.new((0.9, 0.8, 1.0)).textured(texture)
    glass = Dielectric.new((0.9, 0.95, 1.0), 1.5, None)
    parts = []
    lp, ln = _quad((-6.0, 12.0, -6.0), (6.0, 12.0, -6.0), (6.0, 12.0, 6.0), (-6.0, 12.0, 6.0))
    parts.append(Model.new(lp.astype(F), ln.astype(F), Emissive.new((12.0, 11.0, 9.0)), None, "light"))
    parts.append(_placed(*_quad((-30.0, -20.0, -20.0), (30.0, -20.0, -20.0), (30.0, 25.0, -20.0), (-30.0, 25.0, -20.0)),
                         Lambertian.new((0.7, 0.7, 0.7)), (1, -7, -3, 2), "back"))
    pa, na = _quad((-10.0, -20.0, 20.0), (-40.0, -20.0, 20.0), (-40.0, 30.0, 20.0), (-10.0, 30.0, 20.0))
    parts.append(_placed(pa, na, wall, (3, -1, 2, 4), "wall_a", uvs=const_uvs(2, 0.0, 0.0)))
    pb, nb = _quad((20.0, -20.0, 20.0), (-10.0, -20.0, 20.0), (-10.0, 30.0, 20.0), (20.0, 30.0, 20.0))
    parts.append(_placed(pb, nb, wall, (1, -6, -5, 4), "wall_b", uvs=const_uvs(2, 0.5, 0.0)))
    parts.append(_placed(*_quad((-9.0, -2.0, -12.0), (-1.0, -2.0, -12.0), (-1.0, 6.0, -12.0), (-9.0, 6.0, -12.0)),
                         Specular.new((0.9, 0.8, 0.7)), (2, 3, -5, 7), "mirror"))
    parts.append(_placed(*_box((4.0, -3.0, 2.0), (8.0, 2.0, 3.0)), glass, (1, -7, 2, 3), "slab"))
    # the prism's cross-section in (y, z): (-4, 4), (-1, 4), (-4, 1); front face z = 4, bottom face y = -4, hypotenuse z = y + 5
    x0, x1 = -1.0, 3.0
    a0, b0, c0 = (x0, -4.0, 4.0), (x0, -1.0, 4.0), (x0, -4.0, 1.0)
    a1, b1, c1 = (x1, -4.0, 4.0), (x1, -1.0, 4.0), (x1, -4.0, 1.0)
    parts.append(_placed(*_solid([(a0, a1, b1, b0), (a0, c0, c1, a1), (b0, b1, c1, c0), (a0, b0, c0), (a1, c1, b1)]), glass, (5, 1, 1, 7), "prism"))
    parts.append(_placed(*_quad((-40.0, -7.0, 2.0), (-4.0, -7.0, 2.0), (-4.0, -7.0, -18.0), (-40.0, -7.0, -18.0)),
                         Specular.new((0.95, 0.95, 0.9)), (1, -7, -3, 2), "lower"))
    parts.append(_placed(*_quad((-40.0, -6.0, 2.0), (-40.0, -6.9, -18.0), (-4.0, -6.9, -18.0), (-4.0, -6.0, 2.0)),
                         Specular.new((0.9, 0.95, 0.95)), (3, -1, 2, 4), "upper"))
    parts.append(_placed(*_quad((-3.0, -9.0, 8.0), (12.0, -9.0, 8.0), (12.0, -9.0, -20.0), (-3.0, -9.0, -20.0)),
                         GGX.new_metal((0.9, 0.6, 0.2), 0.05), (2, 3, -5, 7), "floor"))
    assert [m.name for m in parts] == ROOM_MODELS
    cam = camera if camera is not None else Camera.new((0.0, 0.0, 12.0), (0.0, -1.0, -2.0), 70.0, w / h)
    return SceneDesc.new(parts, cam, "follow room")


def case_counts(g, max_hops):
    """how many pixels of a chains() result are of each kind the room was built for"""
    hit = g["model"] != MISS
    hops = g["hops"]
    slab = ROOM_MODELS.index("slab")
    hm, hf = g["hop_model"], g["hop_front"]
    # in through one of the pane's faces and straight out through the parallel one (not its rim, not reflected inside)
    via_slab = np.zeros(len(hops), bool)
    if max_hops >= 2:
        parallel = (g["hop_normal"][:, 0].astype(np.float64) * g["hop_normal"][:, 1]).sum(axis=1) > 0.999
        via_slab = (hm[:, 0] == slab) & (hf[:, 0] == 1) & (hm[:, 1] == slab) & (hf[:, 1] == 0) & (hm[:, 2] != slab) & (hops >= 2) & parallel
    last = np.take_along_axis(hm, hops[:, None].astype(np.int64), axis=1)[:, 0]
    delta = [ROOM_MODELS.index(k) for k in ("mirror", "slab", "prism", "lower", "upper")]     # the models of mirror and glass
    return dict(followed_hit=int((hit & (hops > 0)).sum()), capped=int((hit & (hops == max_hops) & np.isin(last, delta)).sum()),
                followed_miss=int((~hit & (hops > 0)).sum()), tir=int(g["tir"].sum()), via_slab=int(via_slab.sum())), via_slab
