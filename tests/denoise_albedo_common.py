"""Shared by tests/test_denoise_albedo_host.py and tests/test_gpu_denoise_albedo.py: the demodulated filter (pt_denoise_albedo /
pt_post_denoise_albedo) restated in numpy float32 from include/pt_api.h, operation for operation, out of test_denoise_host's helpers, with a
level loop of its own that takes (colour, variance); and the scenes and images the two suites use.  Nothing here calls the library."""
import numpy as np

from test_denoise_host import EPS, HK, KB, MISS, F, _exp, _normal_w, _plane, _shift, lum, params

FLOOR = F(2.0 ** -10)


def divisor(albedo, model):
    """k: (1, 1, 1) for a miss, else the albedo floored at 2^-10 per channel"""
    albedo = np.asarray(albedo, F)
    k = np.where(albedo > FLOOR, albedo, FLOOR).astype(F)
    return np.where((np.asarray(model, np.uint32) == MISS)[..., None], F(1), k).astype(F)


def _neighbours(valid, model):
    def neighbour(dx, dy):
        """per pixel: is p + (dx, dy) p itself or a neighbour of p"""
        if dx == 0 and dy == 0:
            return valid.copy()
        mq, ins = _shift(model, dx, dy, fill=0)
        vq, _ = _shift(valid, dx, dy, fill=False)
        return valid & ins & vq & (mq == model)
    return neighbour


def prepare(acc, model, albedo, sumsq=None):
    """(c', var' or None, k, valid): the demodulated colour, the moments' variance scaled by r * r (None: the spatial pass fills it in)"""
    acc = np.asarray(acc, F); model = np.asarray(model, np.uint32)
    valid = acc[..., 3] != 0
    k = divisor(albedo, model)
    n = acc[..., 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cd = np.where(valid[..., None], (acc[..., :3] / k) / n[..., None], F(0)).astype(F)
        var = None
        if sumsq is not None:
            m = lum(acc) / n
            v = np.asarray(sumsq, F) / n - m * m
            v = np.where(v > 0, v, F(0)).astype(F)
            e2 = v / n
            c = (acc[..., :3] / n[..., None]).astype(F)
            lc = lum(c)
            r = np.where(lc > 0, lum(cd) / lc, F(1)).astype(F)
            var = np.where(valid, (e2 * r) * r, F(0)).astype(F)
    return cd, var, k, valid


def spatial_variance(c, valid, hit, nv, pos, model, log2_sn, sx):
    h, w = c.shape[:2]
    neighbour = _neighbours(valid, model)
    l = lum(c)
    sw = np.zeros((h, w), F); s1 = np.zeros((h, w), F); s2 = np.zeros((h, w), F)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            ok = neighbour(dx, dy)
            lq, _ = _shift(l, dx, dy)
            if dx == 0 and dy == 0:
                wt = np.ones((h, w), F)
            else:
                nq, _ = _shift(nv, dx, dy); xq, _ = _shift(pos, dx, dy)
                g = _normal_w(nv, nq, log2_sn) * _exp(-_plane(nv, pos, xq, sx))
                wt = np.where(hit, g, F(1)).astype(F)
            wt = np.where(ok, wt, F(0)).astype(F)
            with np.errstate(invalid="ignore", over="ignore"):
                sw = np.where(ok, sw + wt, sw); s1 = np.where(ok, s1 + wt * lq, s1); s2 = np.where(ok, s2 + wt * (lq * lq), s2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu = s1 / sw
        v = s2 / sw - mu * mu
    return np.where(valid & (v > 0), v, F(0)).astype(F)


def levels(c, var, valid, hit, nv, pos, model, it, sl, log2_sn, sx):
    """the a-trous levels of include/pt_api.h from (c, var) to the last level's colour"""
    h, w = c.shape[:2]
    neighbour = _neighbours(valid, model)
    for i in range(it):
        s = 1 << i
        sg = np.zeros((h, w), F); sk = np.zeros((h, w), F)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                ok = neighbour(dx, dy)
                vq, _ = _shift(var, dx, dy)
                k = KB[dx + 1] * KB[dy + 1]
                with np.errstate(invalid="ignore", over="ignore"):
                    sg = np.where(ok, sg + k * vq, sg); sk = np.where(ok, sk + k, sk)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            g = sg / sk
            inv = F(1) / (sl * np.sqrt(g) + EPS)
        lp = lum(c)
        sw = np.zeros((h, w), F); sc = np.zeros((h, w, 3), F); sv = np.zeros((h, w), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ok = neighbour(s * dx, s * dy)
                cq, _ = _shift(c, s * dx, s * dy); vq, _ = _shift(var, s * dx, s * dy)
                if dx == 0 and dy == 0:
                    e = np.ones((h, w), F)
                else:
                    nq, _ = _shift(nv, s * dx, s * dy); xq, _ = _shift(pos, s * dx, s * dy)
                    with np.errstate(invalid="ignore", over="ignore"):
                        al = np.abs(lp - lum(cq)) * inv
                        e_hit = _normal_w(nv, nq, log2_sn) * _exp(-(_plane(nv, pos, xq, sx) + al))
                    e_miss = _exp(-al)
                    e = np.where(hit, e_hit, e_miss).astype(F)
                wt = np.where(ok, (HK[dx + 2] * HK[dy + 2]) * e, F(0)).astype(F)
                with np.errstate(invalid="ignore", over="ignore"):
                    sw = np.where(ok, sw + wt, sw)
                    sc = np.where(ok[..., None], sc + wt[..., None] * cq, sc)
                    sv = np.where(ok, sv + (wt * wt) * vq, sv)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            c = np.where(valid[..., None], sc / sw[..., None], F(0)).astype(F)
            var = np.where(valid, sv / (sw * sw), F(0)).astype(F)
    return c


def denoise_albedo(acc, pos, nrm, model, albedo, sumsq=None, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0):
    """the demodulated filter of include/pt_api.h: test_denoise_host.denoise's images and an h x w x 3 albedo -> h x w x 4"""
    it, sl, log2_sn, sx = params(iterations, sigma_luminance, sigma_normal, sigma_plane)
    acc = np.asarray(acc, F); pos = np.asarray(pos, F); nrm = np.asarray(nrm, F); model = np.asarray(model, np.uint32)
    h, w = acc.shape[:2]
    cd, var, k, valid = prepare(acc, model, albedo, sumsq)
    hit = model != MISS
    nv = np.concatenate([nrm, valid[..., None].astype(F)], axis=-1)
    if var is None:
        var = spatial_variance(cd, valid, hit, nv, pos, model, log2_sn, sx)
    c = levels(cd, var, valid, hit, nv, pos, model, it, sl, log2_sn, sx)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.concatenate([c * k, np.ones((h, w, 1), F)], axis=-1)
    return np.where(valid[..., None], out, F(0)).astype(F)


def mean_albedo(sums):
    """A of PT_ALBEDO_MEAN from pt_read_albedo's (sum r, sum g, sum b, n)"""
    sums = np.asarray(sums, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (sums[..., :3] / sums[..., 3:4]).astype(F)


def random_albedo(rng, h, w):
    """albedo in (0, 2) with some channels forced to 0 and some pixels forced to 1"""
    al = (rng.random((h, w, 3)).astype(F) * F(2)).astype(F)
    al[rng.random((h, w, 3)) < 0.08] = 0
    al[rng.random((h, w)) < 0.1] = 1
    return al


def checker_image(W=48, H=32, square=4, spp=4, seed=1):
    """The issue's flat one-model image: a checker albedo (0.875 / 0.125, green halved) times a smooth irradiance ramp E = 0.5 + x / W, spp
    noisy samples d = E * |1 + 0.6 N|.  Returns acc, pos, nrm, model, albedo, truth."""
    rng = np.random.default_rng(seed)
    x = np.arange(W, dtype=F)[None, :, None]
    E = np.broadcast_to(F(0.5) + x / F(W), (H, W, 1)).astype(F)
    chk = ((np.arange(H)[:, None] // square + np.arange(W)[None, :] // square) % 2).astype(bool)
    a = np.where(chk, F(0.125), F(0.875)).astype(F)
    albedo = np.stack([a, a * F(0.5), a], -1).astype(F)
    acc = np.zeros((H, W, 4), F)
    for _ in range(spp):
        d = (E * np.abs(F(1) + F(0.6) * rng.normal(size=(H, W, 1)).astype(F))).astype(F)
        acc[..., :3] += albedo * d
        acc[..., 3] += F(1)
    pos = np.zeros((H, W, 4), F); pos[..., 0] = np.arange(W, dtype=F)[None]; pos[..., 1] = np.arange(H, dtype=F)[:, None]; pos[..., 3] = F(5)
    nrm = np.zeros((H, W, 3), F); nrm[..., 2] = 1
    return acc, pos, nrm, np.zeros((H, W), np.uint32), albedo, (albedo * E).astype(F)


def rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a)[..., :3].astype(np.float64) - np.asarray(ref)[..., :3].astype(np.float64)) ** 2)))


def checker_scene(width, height):
    """A checker-textured Lambertian floor and back wall (one 8 x 8 texture of texels 0.9 / 0.1: 8 squares across each), lit by a light above
    the view; open to the sides."""
    from path_tracer_amd.scene_desc import Camera, Emissive, Lambertian, Model, SceneDesc, Texture
    from textures_common import quad
    t = np.where((np.add.outer(np.arange(8), np.arange(8)) % 2).astype(bool), F(0.1), F(0.9)).astype(F)
    lam = Lambertian.new((1.0, 1.0, 1.0)).textured(Texture.new(np.repeat(t[..., None], 3, -1)))
    fp, fn = quad((-8.0, -4.0, -8.0), (-8.0, -4.0, 8.0), (8.0, -4.0, 8.0), (8.0, -4.0, -8.0))
    bp, bn = quad((-8.0, -4.0, -8.0), (8.0, -4.0, -8.0), (8.0, 6.0, -8.0), (-8.0, 6.0, -8.0))
    uv = np.array([[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]], F)
    lp, ln = quad((-3.0, 5.9, -3.0), (3.0, 5.9, -3.0), (3.0, 5.9, 3.0), (-3.0, 5.9, 3.0))
    models = [Model.new(lp, ln, Emissive.new((6.0, 5.0, 4.0)), None, "light"), Model.new(fp, fn, lam, None, "floor", uvs=uv),
              Model.new(bp, bn, lam, None, "back", uvs=uv)]
    return SceneDesc.new(models, Camera.new((1.0, 1.5, 9.0), (0.0, -1.0, -2.0), 65.0, width / height), "checker floor and wall")
