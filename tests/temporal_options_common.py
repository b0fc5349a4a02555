"""Shared by tests/test_temporal_options_host.py and tests/test_gpu_temporal_options.py: the options of the temporal stage (pt_temporal_options'
rescue, length_rule and demodulate) restated in numpy float32 from include/pt_api.h, operation for operation, on top of temporal_common's taps,
variance and levels; and the cases the two suites use.  Nothing here calls the library."""
import numpy as np

import denoise_common
from denoise_common import levels
from temporal_common import MAXN, MISS, F, _dot, lum, params, random_case, taps, tparams, variance


def _fold(acc, tap_list, gate, prev, cur, xp, npv, nmin_, pmax):
    """steps 2 and 3 over tap_list for the pixels of `gate`; acc = [sw, sc, s1, s2, nmin, sN, count] is folded in place"""
    H, M, X, Nq, Mq = prev
    _, pos, _, model = cur
    h, w = model.shape
    hit = model != MISS
    sw, sc, s1, s2, nmin, sn, count = acc
    for qx, qy, b, listed in tap_list:
        inside = gate & listed & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        ix = np.clip(qx, 0, w - 1); iy = np.clip(qy, 0, h - 1)
        Hq = H[iy, ix]; Mo = M[iy, ix]; Xq = X[iy, ix]; nq = Nq[iy, ix]
        with np.errstate(invalid="ignore", over="ignore"):
            ok = inside & (b > 0) & (Hq[..., 3] > 0) & (Mq[iy, ix] == model)
            nd = _dot(npv, nq)
            pd = np.abs(_dot(npv, Xq[..., :3] - xp[..., :3]))
            ok &= ~hit | ((nd >= nmin_) & (pd <= pmax * pos[..., 3]))
            sw = np.where(ok, sw + b, sw)
            sc = np.where(ok[..., None], sc + b[..., None] * Hq[..., :3], sc)
            s1 = np.where(ok, s1 + b * Mo[..., 0], s1)
            s2 = np.where(ok, s2 + b * Mo[..., 1], s2)
            nmin = np.where(ok, np.minimum(nmin, Hq[..., 3]), nmin)
            sn = np.where(ok, sn + b * Hq[..., 3], sn)
        count = count + ok
    acc[:] = [sw.astype(F), sc.astype(F), s1.astype(F), s2.astype(F), nmin.astype(F), sn.astype(F), count]


def fractions(w, h, velocity):
    """step 1's (x0, y0, tx, ty, listed) of every pixel under a velocity"""
    xs = np.broadcast_to(np.arange(w)[None, :], (h, w)); ys = np.broadcast_to(np.arange(h)[:, None], (h, w))
    x0, y0, _, listed = taps(w, h, velocity)[0]                 # (x0, y0) and the listed test are step 1's
    vel = np.asarray(velocity, F)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = ((xs.astype(F) + F(0.5)) / F(w) - vel[..., 0]) * F(w) - F(0.5)
        fy = ((ys.astype(F) + F(0.5)) / F(h) - vel[..., 1]) * F(h) - F(0.5)
    fx = np.where(listed, fx, F(0)).astype(F); fy = np.where(listed, fy, F(0)).astype(F)
    return x0, y0, (fx - np.floor(fx)).astype(F), (fy - np.floor(fy)).astype(F), listed


def rescue_centre(w, h, velocity):
    """step 3b's centre c of every pixel and whether step 1's list has an entry: (cx, cy, listed)"""
    if velocity is None:
        xs = np.broadcast_to(np.arange(w)[None, :], (h, w)); ys = np.broadcast_to(np.arange(h)[:, None], (h, w))
        return xs, ys, np.ones((h, w), bool)
    x0, y0, tx, ty, listed = fractions(w, h, velocity)
    return x0 + (tx >= F(0.5)), y0 + (ty >= F(0.5)), listed


def reproject(prev, cur, xprev=None, nprev=None, velocity=None, alpha=0.0, alpha_moments=0.0, normal_min=0.0, plane_max=0.0, rescue=0, length_rule=0,
              stats=None):
    """steps 1-4 with 3b and the length rule.  Arguments and result as temporal_common.reproject's, whose bits this gives with both options 0.
    stats (a dict): `lost` pixels whose listed taps all failed, `rescue_taps` the valid rescue taps of every pixel (h x w), `restarted`."""
    al, am_, nmin_, pmax = tparams(alpha, alpha_moments, normal_min, plane_max)
    prev = tuple(np.asarray(a, t) for a, t in zip(prev, (F,) * 4 + (np.uint32,)))
    cur = tuple(np.asarray(a, t) for a, t in zip(cur, (F,) * 3 + (np.uint32,)))
    inp, pos, nrm, model = cur
    h, w = model.shape
    xp = pos if xprev is None else np.asarray(xprev, F)
    npv = nrm if nprev is None else np.asarray(nprev, F)
    acc = [np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F), np.full((h, w), np.inf, F), np.zeros((h, w), F),
           np.zeros((h, w), np.int32)]
    everywhere = np.ones((h, w), bool)
    _fold(acc, taps(w, h, velocity), everywhere, prev, cur, xp, npv, nmin_, pmax)
    cx, cy, listed = rescue_centre(w, h, velocity)
    lost = listed & (acc[0] == 0)
    rescue_taps = np.zeros((h, w), np.int32)
    if rescue:
        before = acc[6]
        one = np.ones((h, w), F)
        nine = [(cx + dx, cy + dy, one, listed) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        _fold(acc, nine, lost, prev, cur, xp, npv, nmin_, pmax)
        rescue_taps = acc[6] - before
    sw, sc, s1, s2, nmin, sn, _ = acc
    has = sw > 0
    l = lum(inp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hist = sc / sw[..., None]; m1 = s1 / sw; m2 = s2 / sw
        base = np.floor(sn / sw + F(0.5)).astype(F) if length_rule else nmin
        n = np.minimum(base + F(1), MAXN)
        rn = F(1) / n
        a = np.where(al > rn, al, rn).astype(F); am = np.where(am_ > rn, am_, rn).astype(F)
        c = hist * (F(1) - a)[..., None] + inp[..., :3] * a[..., None]
        mu1 = m1 * (F(1) - am) + l * am
        mu2 = m2 * (F(1) - am) + (l * l) * am
    C = np.where(has[..., None], c, inp[..., :3]).astype(F)
    N = np.where(has, n, F(1)).astype(F)
    mom = np.stack([np.where(has, mu1, l), np.where(has, mu2, l * l)], -1).astype(F)
    if stats is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            stats.update(lost=lost, rescue_taps=rescue_taps, restarted=~has, listed=listed, centre=(cx, cy), mean_length=(sn / sw).astype(F), nmin=nmin)
    return np.concatenate([C, N[..., None]], -1).astype(F), mom, np.where(has, a, F(1)).astype(F)


def post_temporal(prev, cur, xprev=None, nprev=None, velocity=None, alpha=0.0, alpha_moments=0.0, normal_min=0.0, plane_max=0.0, sigma_normal=0,
                  sigma_plane=0.0, rescue=0, length_rule=0, stats=None):
    """pt_post_temporal under the two options it honours -> (H, M, variance)"""
    cn, mom, _ = reproject(prev, cur, xprev, nprev, velocity, alpha, alpha_moments, normal_min, plane_max, rescue, length_rule, stats)
    return cn, mom, variance(cn, mom, cur, alpha, sigma_normal, sigma_plane)


def divisor(model, albedo):
    """pt_denoise_albedo's k: (1, 1, 1) for a miss, else the albedo floored at 2^-10 per channel"""
    return denoise_common.divisor(np.asarray(albedo, F)[..., :3], model)


def frame_temporal(prev, cur, xprev=None, nprev=None, velocity=None, feedback=0, alpha=0.0, alpha_moments=0.0, normal_min=0.0, plane_max=0.0,
                   iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, rescue=0, length_rule=0, albedo=None, stats=None):
    """steps 1-7 of pt_frame_temporal under the options; albedo (h x w x 3, the frame's albedo guide) selects demodulate = 1.
    -> (the state to hand the next step as prev, variance, the filtered frame h x w x 4)"""
    inp, pos, nrm, model = (np.asarray(a, t) for a, t in zip(cur, (F,) * 3 + (np.uint32,)))
    h, w = model.shape
    k = None
    if albedo is not None:
        k = divisor(model, albedo)
        inp = np.concatenate([(inp[..., :3] / k).astype(F), inp[..., 3:]], -1).astype(F)
    cur = (inp, pos, nrm, model)
    cn, mom, var = post_temporal(prev, cur, xprev, nprev, velocity, alpha, alpha_moments, normal_min, plane_max, sigma_normal, sigma_plane, rescue, length_rule,
                                 stats)
    it, sl, log2_sn, sx = params(iterations, sigma_luminance, sigma_normal, sigma_plane)
    valid = np.ones((h, w), bool)
    nv = np.concatenate([nrm, np.ones((h, w, 1), F)], -1)
    c = np.ascontiguousarray(cn[..., :3])
    hit = model != MISS
    out = levels(c, var, valid, hit, nv, pos, model, it, sl, log2_sn, sx)
    if k is not None:
        out = (out * k).astype(F)
    H = cn.copy()
    if feedback:
        H[..., :3] = levels(c, var, valid, hit, nv, pos, model, 1, sl, log2_sn, sx)     # level 0's output, before any multiplication
    state = (H, mom, pos.copy(), nrm.copy(), model.copy())
    return state, var, np.concatenate([out, np.ones((h, w, 1), F)], -1).astype(F)


# ---------------------------------------------------------------- cases
def plane(w, h, model=0):
    """one plane facing the camera: every tap passes the normal and plane tests"""
    pos = np.zeros((h, w, 4), F); pos[..., 0] = np.arange(w, dtype=F)[None]; pos[..., 1] = np.arange(h, dtype=F)[:, None]; pos[..., 3] = 5
    nrm = np.zeros((h, w, 3), F); nrm[..., 2] = 1
    return pos, nrm, np.full((h, w), model, np.uint32)


def options_case(rng, w, h):
    """temporal_common.random_case made harsher for the options: more holes and model flips, so that many pixels lose every listed tap while a
    neighbour still stands; velocities that land tx and ty exactly on 0.5 and centres at -1 and w; N of 65534 and 65535 side by side; runs of
    equal N.  Returns prev, cur, xprev, nprev, velocity."""
    prev, cur, xprev, nprev, vel = random_case(rng, w, h)
    H, M, px, pn, pm = (a.copy() for a in prev)
    model = cur[3]
    # a third of the pixels lose their history or see another model before; blocks of equal N make sN / sw a mean of equals
    H[rng.random((h, w)) < 0.2, 3] = 0
    flip = rng.random((h, w)) < 0.15
    pm[flip] = (pm[flip] + 2) % 4
    same = rng.random((h, w)) < 0.3
    H[same & (H[..., 3] > 0), 3] = F(rng.integers(3, 30))
    # half-pixel velocities: fx = x - 0.5 or x + 0.5 exactly where w and h are powers of two, else near it
    half = rng.random((h, w)) < 0.2
    vel[half, 0] = F(0.5) / F(w) * rng.choice([-1, 1], half.sum()).astype(F)
    vel[half, 1] = F(0.5) / F(h) * rng.choice([-1, 1, 3], half.sum()).astype(F)
    # the first and last columns reproject to fx in [-1, -0.5) and [w - 0.5, w): the centres -1 and w
    vel[:, 0, 0] = F(0.75) / F(w); vel[:, 0, 1] = 0
    vel[:, w - 1, 0] = F(-0.75) / F(w); vel[:, w - 1, 1] = 0
    return (H, M, px, pn, pm), cur, xprev, nprev, vel
