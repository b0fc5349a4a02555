"""The one numpy float32 restatement of the denoiser's parts (include/pt_api.h, operation for operation, with exp taken from the oracle's
independently written exp_det, math_batch fn 1): what a tap weighs, the preparation with or without an albedo, the 7 x 7 spatial variance
and the a-trous levels.  test_denoise_host.denoise, denoise_albedo_common.denoise_albedo and the temporal restatements are compositions of
them.  Nothing here calls the library."""
import numpy as np

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
EPS = F(1e-6)
KB = (F(0.25), F(0.5), F(0.25))
HK = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
FLOOR = F(2.0 ** -10)


def _exp(x):
    from oracle import oracle as O
    x = np.ascontiguousarray(x, F)
    return O.math_batch(1, x.ravel())[0].reshape(x.shape)


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where inside the image, else fill; and the inside mask"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ins = np.zeros((h, w), bool)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = a[ys, xs]
        ins[yd, xd] = True
    return out, ins


def _normal_w(n_p, n_q, log2_sn):
    nd = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
    wn = np.where(nd > 0, nd, F(0)).astype(F)
    for _ in range(log2_sn):
        wn = wn * wn
    return wn


def _plane(n_p, x_p, x_q, sx):
    d = x_q[..., :3] - x_p[..., :3]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    nd = np.abs((n_p[..., 0] * d[..., 0] + n_p[..., 1] * d[..., 1]) + n_p[..., 2] * d[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        ax = nd / (sx * np.sqrt(d2))
    return np.where(d2 > 0, ax, F(0)).astype(F)


def params(iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0):
    """pt_denoise_params with the defaults filled in: (levels, sigma_l, log2 sigma_n, sigma_x)"""
    it = iterations or 5
    sn = sigma_normal or 128
    return it, F(sigma_luminance or 4.0), int(sn).bit_length() - 1, F(sigma_plane or 1.0)


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


def prepare(acc, model, albedo=None, sumsq=None):
    """(c, var or None, k or None, valid).  Plain (albedo None): the colour acc.rgb / acc.w and the moments' variance e2.  With an albedo: the
    demodulated colour c' = (acc.rgb / k) / acc.w and e2 scaled by r * r.  var None: no moments, the spatial pass fills it in"""
    acc = np.asarray(acc, F); model = np.asarray(model, np.uint32)
    valid = acc[..., 3] != 0
    k = None if albedo is None else divisor(albedo, model)
    n = acc[..., 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = np.where(valid[..., None], acc[..., :3] / n[..., None], F(0)).astype(F)
        cd = c if k is None else np.where(valid[..., None], (acc[..., :3] / k) / n[..., None], F(0)).astype(F)
        var = None
        if sumsq is not None:
            m = lum(acc) / n
            v = np.asarray(sumsq, F) / n - m * m
            v = np.where(v > 0, v, F(0)).astype(F)
            e2 = v / n
            if k is not None:
                lc = lum((acc[..., :3] / n[..., None]).astype(F))
                r = np.where(lc > 0, lum(cd) / lc, F(1)).astype(F)
                e2 = (e2 * r) * r
            var = np.where(valid, e2, F(0)).astype(F)
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


def filtered(acc, pos, nrm, model, albedo, sumsq, iterations, sigma_luminance, sigma_normal, sigma_plane):
    """prepare, the spatial variance where there are no moments, the levels, and with an albedo the multiplication by k -> h x w x 4"""
    it, sl, log2_sn, sx = params(iterations, sigma_luminance, sigma_normal, sigma_plane)
    acc = np.asarray(acc, F); pos = np.asarray(pos, F); nrm = np.asarray(nrm, F); model = np.asarray(model, np.uint32)
    h, w = acc.shape[:2]
    c, var, k, valid = prepare(acc, model, albedo, sumsq)
    hit = model != MISS
    nv = np.concatenate([nrm, valid[..., None].astype(F)], axis=-1)
    if var is None:
        var = spatial_variance(c, valid, hit, nv, pos, model, log2_sn, sx)
    c = levels(c, var, valid, hit, nv, pos, model, it, sl, log2_sn, sx)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.concatenate([c if k is None else c * k, np.ones((h, w, 1), F)], axis=-1)
    return np.where(valid[..., None], out, F(0)).astype(F)
