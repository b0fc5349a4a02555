"""Shared by tests/test_temporal_host.py and tests/test_gpu_temporal.py: the temporal stage (pt_frame_temporal / pt_post_temporal) restated in
numpy float32 from include/pt_api.h, operation for operation, on top of the existing restatements of the spatial variance and the levels; and
the random cases the two suites use.  Nothing here calls the library."""
import numpy as np

from denoise_common import MISS, F, _shift, levels, lum, params, spatial_variance  # noqa: F401  (_shift: the levels' and the variance's neighbourhoods)

MAXN = F(65535)
MOMENTS_N = F(4)


def tparams(alpha=0.0, alpha_moments=0.0, normal_min=0.0, plane_max=0.0):
    """pt_temporal_params with the defaults filled in"""
    return F(alpha or 0.2), F(alpha_moments or 0.2), F(normal_min or 0.9), F(plane_max or 0.02)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def carried_normal(nrm, inst, inv12, prev12, moved):
    """nprev: the normal through the linear parts of its instance's inverse and previous forward matrix where `moved[instance]`, else as it is"""
    nrm = np.asarray(nrm, F); inst = np.asarray(inst, np.uint32)
    out = nrm.copy()
    n = len(moved)
    sel = inst < n
    sel[sel] = np.asarray(moved, bool)[inst[sel]]
    if not sel.any():
        return out
    v = nrm[sel]
    inv = np.asarray(inv12, F).reshape(-1, 3, 4)[inst[sel]]; prv = np.asarray(prev12, F).reshape(-1, 3, 4)[inst[sel]]
    o = np.stack([(inv[:, k, 0] * v[:, 0] + inv[:, k, 1] * v[:, 1]) + inv[:, k, 2] * v[:, 2] for k in range(3)], -1).astype(F)
    q = np.stack([(prv[:, k, 0] * o[:, 0] + prv[:, k, 1] * o[:, 1]) + prv[:, k, 2] * o[:, 2] for k in range(3)], -1).astype(F)
    out[sel] = q
    return out


def taps(w, h, velocity):
    """step 1: a list of up to four (qx, qy, b, listed) image-sized arrays, in list order"""
    xs = np.broadcast_to(np.arange(w)[None, :], (h, w)); ys = np.broadcast_to(np.arange(h)[:, None], (h, w))
    if velocity is None:
        return [(xs, ys, np.ones((h, w), F), np.ones((h, w), bool))]
    vel = np.asarray(velocity, F)
    with np.errstate(invalid="ignore", over="ignore"):
        cu = (xs.astype(F) + F(0.5)) / F(w); cv = (ys.astype(F) + F(0.5)) / F(h)
        pu = cu - vel[..., 0]; pv = cv - vel[..., 1]
        fx = pu * F(w) - F(0.5); fy = pv * F(h) - F(0.5)
        listed = (fx >= F(-1)) & (fx < F(w)) & (fy >= F(-1)) & (fy < F(h))
    fx = np.where(listed, fx, F(0)).astype(F); fy = np.where(listed, fy, F(0)).astype(F)
    bx = np.floor(fx); by = np.floor(fy)
    tx = fx - bx; ty = fy - by
    x0 = bx.astype(np.int64); y0 = by.astype(np.int64)
    out = []
    for j in (0, 1):
        for i in (0, 1):
            b = ((tx if i else F(1) - tx) * (ty if j else F(1) - ty)).astype(F)
            out.append((x0 + i, y0 + j, b, listed))
    return out


def reproject(prev, cur, xprev=None, nprev=None, velocity=None, alpha=0.0, alpha_moments=0.0, normal_min=0.0, plane_max=0.0, stats=None):
    """steps 1-4.  prev = (H h x w x 4, M h x w x 2, X' h x w x 4, n' h x w x 3, m' h x w), cur = (input h x w x 4, position, normal, model).
    Returns (C | N, (mu1, mu2), a).  stats (a dict): the number of pixels with no valid tap and with four."""
    al, am_, nmin_, pmax = tparams(alpha, alpha_moments, normal_min, plane_max)
    H, M, X, Nq, Mq = (np.asarray(a, t) for a, t in zip(prev, (F,) * 4 + (np.uint32,)))
    inp, pos, nrm, model = (np.asarray(a, t) for a, t in zip(cur, (F,) * 3 + (np.uint32,)))
    h, w = model.shape
    xp = pos if xprev is None else np.asarray(xprev, F)
    npv = nrm if nprev is None else np.asarray(nprev, F)
    hit = model != MISS
    sw = np.zeros((h, w), F); sc = np.zeros((h, w, 3), F); s1 = np.zeros((h, w), F); s2 = np.zeros((h, w), F)
    nmin = np.full((h, w), np.inf, F); count = np.zeros((h, w), np.int32)
    for qx, qy, b, listed in taps(w, h, velocity):
        inside = listed & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        ix = np.clip(qx, 0, w - 1); iy = np.clip(qy, 0, h - 1)
        Hq = H[iy, ix]; Mo = M[iy, ix]; Xq = X[iy, ix]; nq = Nq[iy, ix]
        with np.errstate(invalid="ignore", over="ignore"):
            ok = inside & (b > 0) & (Hq[..., 3] > 0) & (Mq[iy, ix] == model)
            nd = _dot(npv, nq)
            d = Xq[..., :3] - xp[..., :3]
            pd = np.abs(_dot(npv, d))
            ok &= ~hit | ((nd >= nmin_) & (pd <= pmax * pos[..., 3]))
            sw = np.where(ok, sw + b, sw)
            sc = np.where(ok[..., None], sc + b[..., None] * Hq[..., :3], sc)
            s1 = np.where(ok, s1 + b * Mo[..., 0], s1)
            s2 = np.where(ok, s2 + b * Mo[..., 1], s2)
            nmin = np.where(ok, np.minimum(nmin, Hq[..., 3]), nmin)
        count += ok
    has = sw > 0
    l = lum(inp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hist = sc / sw[..., None]; m1 = s1 / sw; m2 = s2 / sw
        n = np.minimum(nmin + F(1), MAXN)
        rn = F(1) / n
        a = np.where(al > rn, al, rn).astype(F); am = np.where(am_ > rn, am_, rn).astype(F)
        c = hist * (F(1) - a)[..., None] + inp[..., :3] * a[..., None]
        mu1 = m1 * (F(1) - am) + l * am
        mu2 = m2 * (F(1) - am) + (l * l) * am
    C = np.where(has[..., None], c, inp[..., :3]).astype(F)
    N = np.where(has, n, F(1)).astype(F)
    mom = np.stack([np.where(has, mu1, l), np.where(has, mu2, l * l)], -1).astype(F)
    if stats is not None:
        stats["disoccluded"] = int((~has).sum()); stats["four_taps"] = int((count == 4).sum())
    return np.concatenate([C, N[..., None]], -1).astype(F), mom, np.where(has, a, F(1)).astype(F)


def variance(cn, mom, cur, alpha=0.0, sigma_normal=0, sigma_plane=0.0):
    """step 5"""
    al = tparams(alpha)[0]
    _, _, log2_sn, sx = params(0, 0.0, sigma_normal, sigma_plane)
    _, pos, nrm, model = (np.asarray(a, t) for a, t in zip(cur, (F,) * 3 + (np.uint32,)))
    h, w = model.shape
    n = cn[..., 3]
    with np.errstate(invalid="ignore", over="ignore"):
        v = mom[..., 1] - mom[..., 0] * mom[..., 0]
        v = np.where(v > 0, v, F(0)).astype(F)
        rn = F(1) / n
        vm = v * np.where(al > rn, al, rn).astype(F)
    valid = np.ones((h, w), bool)
    nv = np.concatenate([nrm, np.ones((h, w, 1), F)], -1)
    vs = spatial_variance(np.ascontiguousarray(cn[..., :3]), valid, model != MISS, nv, pos, model, log2_sn, sx)
    return np.where(n >= MOMENTS_N, vm, vs).astype(F)


def post_temporal(prev, cur, xprev=None, nprev=None, velocity=None, alpha=0.0, alpha_moments=0.0, normal_min=0.0, plane_max=0.0, sigma_normal=0,
                  sigma_plane=0.0, stats=None):
    """pt_post_temporal: steps 1-5 and the feedback = 0 store -> (H, M, variance)"""
    cn, mom, _ = reproject(prev, cur, xprev, nprev, velocity, alpha, alpha_moments, normal_min, plane_max, stats)
    return cn, mom, variance(cn, mom, cur, alpha, sigma_normal, sigma_plane)


def frame_temporal(prev, cur, xprev=None, nprev=None, velocity=None, feedback=0, alpha=0.0, alpha_moments=0.0, normal_min=0.0, plane_max=0.0,
                   iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, stats=None):
    """steps 1-7 of pt_frame_temporal -> (the state to hand the next step as prev, variance, the filtered frame h x w x 4)"""
    cn, mom, var = post_temporal(prev, cur, xprev, nprev, velocity, alpha, alpha_moments, normal_min, plane_max, sigma_normal, sigma_plane, stats)
    it, sl, log2_sn, sx = params(iterations, sigma_luminance, sigma_normal, sigma_plane)
    _, pos, nrm, model = (np.asarray(a, t) for a, t in zip(cur, (F,) * 3 + (np.uint32,)))
    h, w = model.shape
    valid = np.ones((h, w), bool)
    nv = np.concatenate([nrm, np.ones((h, w, 1), F)], -1)
    c = np.ascontiguousarray(cn[..., :3])
    hit = model != MISS
    out = levels(c, var, valid, hit, nv, pos, model, it, sl, log2_sn, sx)
    H = cn.copy()
    if feedback:
        H[..., :3] = levels(c, var, valid, hit, nv, pos, model, 1, sl, log2_sn, sx)
    state = (H, mom, pos.copy(), nrm.copy(), model.copy())
    return state, var, np.concatenate([out, np.ones((h, w, 1), F)], -1).astype(F)


def empty_state(w, h):
    """no history: N = 0 everywhere"""
    return (np.zeros((h, w, 4), F), np.zeros((h, w, 2), F), np.zeros((h, w, 4), F), np.zeros((h, w, 3), F), np.zeros((h, w), np.uint32))


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def random_case(rng, w, h):
    """A previous state, a current frame and a velocity that between them reach every branch: sub-pixel, whole-pixel and out-of-frame
    velocities, NaN and infinite ones; holes (N = 0), N at 65534 and 65535 and below 4; model mismatches; normals exactly at normal_min and
    just beside it; plane distances exactly at the bound and just beyond; misses.  Returns prev, cur, xprev, nprev, velocity."""
    n_models = 4
    model = rng.integers(0, n_models, (h, w)).astype(np.uint32)
    if w > 4 and h > 4:
        model = np.repeat(np.repeat(model[::4, ::4], 4, 0), 4, 1)[:h, :w].copy()
    model[rng.random((h, w)) < 0.12] = MISS
    # the current frame: planes z = const per model seen along +z, so that most taps pass
    nrm = np.zeros((h, w, 3), F); nrm[..., 2] = 1
    tilt = rng.random((h, w)) < 0.3
    nrm[tilt] = _unit(np.stack([rng.normal(size=tilt.sum()) * 0.2, rng.normal(size=tilt.sum()) * 0.2, np.ones(tilt.sum())], -1))
    pos = np.zeros((h, w, 4), F)
    pos[..., 0] = np.arange(w, dtype=F)[None] * F(0.25); pos[..., 1] = np.arange(h, dtype=F)[:, None] * F(0.25)
    pos[..., 2] = (model % 7).astype(F); pos[..., 3] = F(8) + rng.integers(0, 3, (h, w)).astype(F) * F(4)   # t in {8, 12, 16}
    miss = model == MISS
    nrm[miss] = 0; pos[miss, 3] = F(1e5)
    inp = np.concatenate([rng.random((h, w, 3)).astype(F) * F(2), np.ones((h, w, 1), F)], -1).astype(F)
    # the previous state: the same surfaces, with perturbations
    pm = model.copy()
    flip = rng.random((h, w)) < 0.1
    pm[flip] = (pm[flip] + 1) % n_models
    pn = nrm.copy(); px = pos.copy()
    px[..., :3] += (rng.normal(size=(h, w, 3)) * 0.05).astype(F) * (rng.random((h, w, 1)) < 0.5)
    N = rng.integers(1, 40, (h, w)).astype(F)
    N[rng.random((h, w)) < 0.15] = 0
    N[rng.random((h, w)) < 0.1] = 65534
    N[rng.random((h, w)) < 0.1] = 65535
    N[rng.random((h, w)) < 0.15] = rng.integers(1, 4)
    H = np.concatenate([rng.random((h, w, 3)).astype(F) * F(2), N[..., None]], -1).astype(F)
    mu1 = lum(H); M = np.stack([mu1, mu1 * mu1 * (F(1) + rng.random((h, w)).astype(F))], -1).astype(F)
    # velocities in uv: whole pixels, sub-pixel, far out of frame, NaN, infinite, zero
    vel = np.zeros((h, w, 2), F)
    kind = rng.integers(0, 8, (h, w))
    whole = np.stack([rng.integers(-2, 3, (h, w)) / w, rng.integers(-2, 3, (h, w)) / h], -1).astype(F)
    sub = np.stack([(rng.random((h, w)) * 3 - 1.5) / w, (rng.random((h, w)) * 3 - 1.5) / h], -1).astype(F)
    vel[kind <= 2] = sub[kind <= 2]; vel[kind == 3] = whole[kind == 3]; vel[kind == 4] = sub[kind == 4] * F(0.01)
    vel[kind == 5] = F(3.0) * np.sign(sub[kind == 5] + F(1e-9))
    odd = rng.random((h, w))
    vel[odd < 0.03, 0] = np.nan; vel[(odd >= 0.03) & (odd < 0.06), 1] = np.inf; vel[(odd >= 0.06) & (odd < 0.08), 0] = -np.inf
    # previous normals exactly at the bound: n' = (s, 0, c) with c = normal_min to the bit for the untilted current normal (0, 0, 1)
    nmin_ = tparams()[2]
    edge = (rng.random((h, w)) < 0.15) & ~tilt & ~miss
    for c in (nmin_, np.nextafter(nmin_, F(0)), np.nextafter(nmin_, F(2))):
        sel = edge & (rng.random((h, w)) < 0.4)
        pn[sel] = np.array([np.sqrt(F(1) - c * c), 0, c], F)
    # previous positions exactly at the plane bound plane_max * t (t of the CURRENT pixel at rest; under a velocity the tap lands elsewhere
    # and the case is one more perturbation): dz = bound, its neighbour floats, and 0
    pmax = tparams()[3]
    for scale in (F(1), np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0))):
        sel = (rng.random((h, w)) < 0.1) & ~tilt & ~miss
        pos[sel, 2] = 0                                      # so that the difference X'.z - x.z is the bound itself, with no rounding
        px[sel, 2] = (pmax * pos[sel, 3]) * scale
        px[sel, 0] = pos[sel, 0]; px[sel, 1] = pos[sel, 1]; pn[sel] = nrm[sel]
    xprev = pos.copy(); nprev = nrm.copy()
    mv = (rng.random((h, w)) < 0.2) & ~miss
    xprev[mv, :3] += (rng.normal(size=(mv.sum(), 3)) * 0.02).astype(F)
    nprev[mv] = _unit(nprev[mv] + (rng.normal(size=(mv.sum(), 3)) * 0.05).astype(F))
    return (H, M, px, pn, pm), (inp, pos, nrm, model), xprev, nprev, vel
