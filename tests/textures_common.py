"""Shared by tests/test_textures_host.py and tests/test_gpu_textures.py: the definition of the textured surface colour (include/pt_api.h)
restated in numpy, every product, sum and difference ONE np.float32 operation in the order the header writes them, and the scenes the tests
render.  Nothing here calls the library."""
import numpy as np

from path_tracer_amd.scene_desc import (EMISSIVE, GGX, IDENTITY_3x4, Camera, Emissive, Lambertian, Material, Model, SceneDesc, Texture,
                                        Volume)

F = np.float32


def as_u32(x):
    """Rust's `f32 as u32`: NaN and negatives 0, 2^32 and above u32::MAX, else truncation"""
    x = np.asarray(x, F)
    out = np.zeros(x.shape, np.uint64)
    ok = x > F(0.0)                                   # (false for NaN)
    big = ok & (x >= F(4294967296.0))
    mid = ok & ~big
    out[big] = 0xFFFFFFFF
    out[mid] = np.trunc(x[mid].astype(np.float64)).astype(np.uint64)
    return out


def bilinear(tex, s, t):
    """get_pixel_bilinear (image_helper.rs:61-88) of tex [h, w, 3] at (s, t) arrays, as the environment lookup evaluates it"""
    tex = np.asarray(tex, F)
    h, w = tex.shape[0], tex.shape[1]
    s = np.asarray(s, F); t = np.asarray(t, F)
    with np.errstate(invalid="ignore", over="ignore"):
        x = F(w) * s
        y = F(h) * t
        x0, y0 = as_u32(x), as_u32(y)
        xf = x - np.trunc(x)
        yf = y - np.trunc(y)
        one64, m32 = np.uint64(1), np.uint64(0xFFFFFFFF)
        xa, xb = x0 % np.uint64(w), ((x0 + one64) & m32) % np.uint64(w)           # (x0 + 1 wraps in u32)
        ya, yb = y0 % np.uint64(h), ((y0 + one64) & m32) % np.uint64(h)
        c00, c01, c10, c11 = tex[ya, xa], tex[yb, xa], tex[ya, xb], tex[yb, xb]
        one = F(1.0)
        w00 = ((one - xf) * (one - yf))[..., None]
        w01 = ((one - xf) * yf)[..., None]
        w10 = (xf * (one - yf))[..., None]
        w11 = (xf * yf)[..., None]
        return ((w00 * c00 + w01 * c01) + w10 * c10) + w11 * c11


def surface_colour(colour, tex, uv3, u, v):
    """colour [3]; tex [h, w, 3] or None; uv3 [n, 3, 2] the hit triangles' UVs (load-order vertices); u, v [n] barycentrics -> [n, 3]"""
    u = np.asarray(u, F); v = np.asarray(v, F)
    colour = np.asarray(colour, F)
    if tex is None:
        return np.broadcast_to(colour, u.shape + (3,)).copy()
    uv3 = np.asarray(uv3, F)
    with np.errstate(invalid="ignore", over="ignore"):
        st = []
        for k in (0, 1):
            a, b, c = uv3[:, 0, k], uv3[:, 1, k], uv3[:, 2, k]
            x = (a + u * (b - a)) + v * (c - a)
            st.append(x - np.floor(x))
        return colour[None, :] * bilinear(tex, st[0], st[1])


def scene_surface_colour(desc, instance_model, instance, prim, u, v):
    """the restated surface colour of hits on a scene description: instance_model[i] = model of world instance i"""
    instance = np.asarray(instance); prim = np.asarray(prim)
    out = np.zeros((len(instance), 3), F)
    models = np.asarray(instance_model)[instance]
    for mi in np.unique(models):
        sel = np.nonzero(models == mi)[0]
        mod = desc.models[int(mi)]
        tex = mod.material.texture
        uv = mod.uvs if mod.uvs is not None else np.zeros((mod.positions.shape[0], 3, 2), F)
        out[sel] = surface_colour(mod.material.colour, None if tex is None else tex.data, uv[prim[sel]], np.asarray(u, F)[sel], np.asarray(v, F)[sel])
    return out


def world_instance_models(desc):
    """model index of every world-TLAS leaf in allocation order (tlas.rs:24-53: models in order, each model's matrices in order)"""
    return np.array([i for i, m in enumerate(desc.models) for _ in range(m.matrices.shape[0])], np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------- geometry
def quad(p0, p1, p2, p3):
    """two triangles (p0 p1 p2), (p0 p2 p3) with the face normal at every vertex; returns positions, normals [2, 3, 3]"""
    p = np.array([[p0, p1, p2], [p0, p2, p3]], F)
    n = np.cross(p[0, 1] - p[0, 0], p[0, 2] - p[0, 0]).astype(np.float64)
    n = (n / np.sqrt((n * n).sum())).astype(F)
    return p, np.broadcast_to(n, p.shape).copy()


def box(lo, hi):
    """12 outward-facing triangles of an axis-aligned box"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    faces = [((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)), ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)),
             ((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), ((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),
             ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0))]
    ps, ns = zip(*(quad(*f) for f in faces))
    return np.concatenate(ps), np.concatenate(ns)


def const_uvs(n_tris, s, t):
    return np.broadcast_to(np.array([s, t], F), (n_tris, 3, 2)).copy()


LOUD = 50.0


def corner_scene(width, height, lens=False, media=True):
    """The texel-corner scene: a closed room of seven wall / floor / box models on two shared textured materials (Lambertian on a 4 x 2
    texture, GGX metal with a tint on a 2 x 2 one), two glass boxes on a third (GGX dielectric with a volume, on the 2 x 2 texture) and a
    light.  Every vertex of a model carries the same texel corner (i/w, j/h), a different one per model; the other texels are LOUD.
    Returns (textured description, the equivalent untextured description: every such model with its own material of colour
    f32(tint * texel)).  media=False leaves the two glass boxes out: a scene without media, which runs the other half of the shading variants."""
    t42 = np.full((2, 4, 3), LOUD, F)
    t22 = np.full((2, 2, 3), LOUD, F)
    quiet42 = {(0, 0): (0.75, 0.7, 0.65), (1, 0): (0.7, 0.15, 0.12), (2, 1): (0.15, 0.6, 0.2), (3, 1): (0.3, 0.35, 0.8), (1, 1): (0.6, 0.6, 0.2)}
    quiet22 = {(0, 0): (0.9, 0.8, 0.5), (1, 0): (0.95, 0.9, 0.85), (1, 1): (0.8, 0.95, 0.9), (0, 1): (0.5, 0.6, 0.9)}
    for (i, j), c in quiet42.items():
        t42[j, i] = c
    for (i, j), c in quiet22.items():
        t22[j, i] = c
    tex42, tex22 = Texture.new(t42), Texture.new(t22)
    lam = Lambertian.new((1.0, 1.0, 1.0)).textured(tex42)
    metal = GGX.new_metal((0.9, 0.75, 0.6), 0.35).textured(tex22)                       # the tint
    glass = GGX.new_dielectric((1.0, 1.0, 1.0), 0.2, 1.5, Volume.new((0.4, 0.1, 0.2), 0.3, 0.5, 0.2)).textured(tex22)
    S = 10.0
    parts = [  # name, geometry, material, texture size, texel corner
        ("floor", quad((-S, -S, -S), (-S, -S, S), (S, -S, S), (S, -S, -S)), lam, (4, 2), (0, 0)),
        ("ceiling", quad((-S, S, -S), (S, S, -S), (S, S, S), (-S, S, S)), lam, (4, 2), (1, 1)),
        ("back", quad((-S, -S, -S), (S, -S, -S), (S, S, -S), (-S, S, -S)), lam, (4, 2), (0, 0)),
        ("left", quad((-S, -S, -S), (-S, S, -S), (-S, S, S), (-S, -S, S)), lam, (4, 2), (1, 0)),
        ("right", quad((S, -S, -S), (S, -S, S), (S, S, S), (S, S, -S)), lam, (4, 2), (2, 1)),
        ("block", box((-6.0, -S, -6.0), (-1.0, -2.0, -1.0)), metal, (2, 2), (0, 0)),
        ("slab", box((2.0, -S, -7.0), (7.0, -6.0, -3.0)), metal, (2, 2), (1, 0)),
        ("tall", box((3.0, -S, 0.0), (6.0, 1.0, 3.0)), lam, (4, 2), (3, 1)),
        ("glass_a", box((-5.0, -S, 1.0), (-2.0, -4.0, 4.0)), glass, (2, 2), (1, 1)),
        ("glass_b", box((-1.0, -S + 0.01, 4.5), (1.5, -6.0, 7.0)), glass, (2, 2), (0, 1)),
    ]
    tex_of = {id(lam): t42, id(metal): t22, id(glass): t22}
    if not media:
        parts = [q for q in parts if q[2] is not glass]
    textured, plain = [], []
    for name, (p, n), mat, (w, h), (i, j) in parts:
        # a general rigid turn on the slab and an extra instance of the block: the lookup goes through the instance's model, not the leaf
        mats = None
        if name == "block":
            second = IDENTITY_3x4.copy(); second[:, 3] = (0.0, 0.0, 9.0)
            mats = np.stack([IDENTITY_3x4, second])
        textured.append(Model.new(p, n, mat, mats, name, uvs=const_uvs(p.shape[0], i / w, j / h)))
        texel = tex_of[id(mat)][j, i]
        col = (np.asarray(mat.colour, F) * texel).astype(F)                             # f32(tint * texel), per component
        plain.append(Model.new(p, n, Material(mat.kind, tuple(float(c) for c in col), mat.roughness, mat.ior, mat.volume), mats, name))
    lp, ln = quad((-2.5, S - 0.05, -2.5), (2.5, S - 0.05, -2.5), (2.5, S - 0.05, 2.5), (-2.5, S - 0.05, 2.5))
    light = Model.new(lp, ln, Emissive.new((14.0, 12.0, 9.0)), None, "light")
    cam = Camera.new((0.5, 0.5, 9.5), (-0.5, -3.0, -2.0), 70.0, width / height, 0.6 if lens else 0.0, 9.0 if lens else 0.0)
    return SceneDesc.new([light] + textured, cam, "texel corners"), SceneDesc.new([light] + plain, cam, "texel corners, untextured")


def varying_scene(width, height):
    """A textured Lambertian floor and back wall whose UVs vary across each triangle (beyond [0, 1), negative, different per vertex) on a
    5 x 3 texture, an untextured grey side wall and an untextured light; open to the sides (misses)."""
    rng = np.random.default_rng(5)
    tex = Texture.new(rng.uniform(0.05, 0.95, (3, 5, 3)).astype(F))
    lam = Lambertian.new((0.9, 0.8, 0.7)).textured(tex)
    fp, fn = quad((-8.0, -4.0, -8.0), (-8.0, -4.0, 8.0), (8.0, -4.0, 8.0), (8.0, -4.0, -8.0))
    bp, bn = quad((-8.0, -4.0, -8.0), (8.0, -4.0, -8.0), (8.0, 6.0, -8.0), (-8.0, 6.0, -8.0))
    f_uv = np.array([[[0.0, 0.0], [0.0, 2.75], [3.5, 2.75]], [[0.0, 0.0], [3.5, 2.75], [3.5, 0.0]]], F)
    b_uv = np.array([[[-1.25, 0.1], [0.7, -0.4], [1.9, 1.3]], [[-1.25, 0.1], [1.9, 1.3], [-0.3, 2.2]]], F)
    sp, sn = quad((-8.0, -4.0, -8.0), (-8.0, 6.0, -8.0), (-8.0, 6.0, 8.0), (-8.0, -4.0, 8.0))
    lp, ln = quad((-3.0, 5.9, -3.0), (3.0, 5.9, -3.0), (3.0, 5.9, 3.0), (-3.0, 5.9, 3.0))
    models = [Model.new(lp, ln, Emissive.new((6.0, 5.0, 4.0)), None, "light"), Model.new(fp, fn, lam, None, "floor", uvs=f_uv),
              Model.new(bp, bn, lam, None, "back", uvs=b_uv), Model.new(sp, sn, Lambertian.new((0.5, 0.5, 0.5)), None, "side")]
    return SceneDesc.new(models, Camera.new((1.0, 1.5, 9.0), (0.0, 0.0, -2.0), 65.0, width / height), "varying uvs")


assert EMISSIVE == 1
