"""Shared by tests/test_probe_radiance_host.py and tests/test_gpu_probe_radiance.py: reflection probes (include/pt_api.h,
pt_set_probe_grid_radiance) restated in numpy, every product, sum, difference, quotient and square root ONE np.float32 operation in the order
the header writes them: the direction and solid angle of a texel, the radiance bake's fold over Oracle.integrate, the GGX prefilter, the
specular lookup on top of probe_grid_common's grids (with probe_depth_common's visibility where depth is set), and the baked sample with the
metal ending over baked_common's oracle-walked chain.  Nothing here calls the library's device code."""
import numpy as np

import baked_common as BC
import guides_follow_common as G
import probe_depth_common as PD
import probe_grid_common as PG
from path_tracer_amd.scene_desc import EMISSIVE, GGX_METAL
from textures_common import scene_surface_colour, world_instance_models

F = np.float32
MISS = PG.MISS
PI = F(3.14159265358979323846)
# how a chain of the baked view ended, with radiance set: probe_grid_common's endings and the metal one on either face
METAL_FRONT, METAL_BACK = 8, 9
ENDINGS = dict(PG.ENDINGS)
ENDINGS.update({METAL_FRONT: "metal, front face", METAL_BACK: "metal, back face"})


# -------------------------------------------------------------------------------------------------------------------------- the direction
def oct_dir(R, texels=None):
    """THE DIRECTION of include/pt_api.h for texels [k] of a map of side R (None: all, in order) -> (dir [k, 3], omega [k]) float32"""
    t = np.arange(R * R) if texels is None else np.asarray(texels, np.int64).reshape(-1)
    iy, ix = t // R, t % R
    one, half, two, fr = F(1.0), F(0.5), F(2.0), F(R)
    px = two * ((ix.astype(F) + half) / fr) - one
    py = two * ((iy.astype(F) + half) / fr) - one
    z = (one - np.abs(px)) - np.abs(py)
    qx = (one - np.abs(py)) * np.where(px >= F(0.0), one, -one).astype(F)
    qy = (one - np.abs(px)) * np.where(py >= F(0.0), one, -one).astype(F)
    low = z < F(0.0)
    px, py = np.where(low, qx, px).astype(F), np.where(low, qy, py).astype(F)
    ln = np.sqrt((px * px + py * py) + z * z)
    assert ln.dtype == F
    d = np.stack([px / ln, py / ln, z / ln], axis=1)
    om = one / ((ln * ln) * ln)
    assert d.dtype == F and om.dtype == F
    return d, om


# ------------------------------------------------------------------------------------------------------------------------------- the bake
def fold(directions, L, R, sums, counts):
    """THE BAKE's fold of one probe's rays, in the order given (sample order): sums [R * R, 3] float32 and counts [R * R] uint32 in place"""
    texel = PD.oct_texel(directions, R)
    L = np.asarray(L, F)
    for s in range(len(texel)):
        k = texel[s]
        counts[k] += 1
        sums[k] = sums[k] + L[s, :3]
    assert sums.dtype == F


def oracle_rays(orc, r, positions, n_samples, max_bounces, first_sample=0, key_base=0):
    """the rays of a probe bake and what they carry: pt_probe_ray's directions (host evaluation) [n, samples, 3] and Oracle.integrate's
    radiance with the stream (key_base + j, s) and one draw consumed [n, samples, 3].  Computed once and shared: it does not depend on R."""
    pos = np.asarray(positions, F).reshape(-1, 3)
    d = np.zeros((pos.shape[0], n_samples, 3), F); L = np.zeros((pos.shape[0], n_samples, 3), F)
    for j in range(pos.shape[0]):
        for s in range(n_samples):
            d[j, s] = r.probe_ray(key_base + j, first_sample + s)[0]
            L[j, s] = orc.integrate(pos[j], d[j, s], key_base + j, first_sample + s, 1, max_bounces=max_bounces)[0][:3]
    return d, L


def fold_rays(d, L, R, sums=None, counts=None):
    """the restated fold of oracle_rays' output (or a slice of its samples) -> (sums [n, R * R, 3], counts [n, R * R])"""
    n = d.shape[0]
    sums = np.zeros((n, R * R, 3), F) if sums is None else np.array(sums, F).reshape(n, R * R, 3)
    counts = np.zeros((n, R * R), np.uint32) if counts is None else np.array(counts, np.uint32).reshape(n, R * R)
    for j in range(n):
        fold(d[j], L[j], R, sums[j], counts[j])
    return sums, counts


# -------------------------------------------------------------------------------------------------------------------------- the prefilter
def ggx_d(alpha, nh):
    """D of THE PREFILTER for cosines nh [k] (ggx_d of the material, which reads the cosine only) -> [k] float32"""
    a = F(alpha)
    with np.errstate(invalid="ignore", divide="ignore"):
        c2 = nh * nh
        x = (a * a) + np.sqrt(F(1.0) - c2) / c2
        d = (a * a) / ((((PI * c2) * c2) * x) * x)
    assert d.dtype == F
    return np.where(nh <= F(0.0), F(0.0), d).astype(F)


def prefilter_weights(R, alpha):
    """(w [i, j] float32, take [i, j]) of THE PREFILTER for a map of side R at one alpha: the weight of input texel j in output texel i and
    whether n.l > 0 lets it in; what the map holds does not enter"""
    dirs, om = oct_dir(R)
    n, l = dirs[:, None, :], dirs[None, :, :]
    nl = (n[..., 0] * l[..., 0] + n[..., 1] * l[..., 1]) + n[..., 2] * l[..., 2]
    h = n + l
    with np.errstate(invalid="ignore", divide="ignore"):
        hl = np.sqrt((h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1]) + h[..., 2] * h[..., 2])
        h = h / hl[..., None]
    nh = (n[..., 0] * h[..., 0] + n[..., 1] * h[..., 1]) + n[..., 2] * h[..., 2]
    nh = np.where(nh > F(1.0), F(1.0), nh).astype(F)
    w = (ggx_d(alpha, nh) * nl) * om[None, :]
    assert w.dtype == F and nl.dtype == F
    return w, nl > F(0.0)


def prefilter(sums, counts, alphas):
    """THE PREFILTER of include/pt_api.h: sums [n, R * R, 3], counts [n, R * R] -> table [n, levels, R * R, 4] float32.  The j loop is the
    header's, ascending; the probes and the output texels i are computed side by side."""
    sums = np.asarray(sums, F); counts = np.asarray(counts, np.uint32)
    n, rr = counts.shape
    R = int(round(np.sqrt(rr)))
    table = np.zeros((n, len(alphas), rr, 4), F)
    filled = counts > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (sums / counts.astype(F)[..., None]).astype(F)                    # [n, j, 3]; an empty texel's is never used
    for l, alpha in enumerate(alphas):
        w, take = prefilter_weights(R, alpha)
        A = np.zeros((n, rr, 3), F); Wt = np.zeros((n, rr), F)
        for j in range(rr):
            use = take[None, :, j] & filled[:, j, None]                          # [n, i]
            with np.errstate(invalid="ignore"):
                A = np.where(use[..., None], A + w[None, :, j, None] * mean[:, None, j, :], A).astype(F)
                Wt = np.where(use, Wt + w[None, :, j], Wt).astype(F)
        pos = Wt > F(0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = A / Wt[..., None]
        table[:, l, :, :3] = np.where(pos[..., None], out, F(0.0))
    return table


def random_maps(n, R, seed, empty=0.3):
    """seeded raw maps: sums [n, R * R, 3] >= 0 and counts [n, R * R], a fraction `empty` of the texels without a sample (their sums are
    junk that must not be read as radiance: non-zero on purpose)"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 40, (n, R * R)).astype(np.uint32)
    counts[rng.uniform(0.0, 1.0, counts.shape) < empty] = 0
    sums = (rng.uniform(0.0, 4.0, (n, R * R, 3)) * np.maximum(counts, 1)[..., None]).astype(F)
    return sums, counts


# ----------------------------------------------------------------------------------------------------------------------------- the lookup
class Radiance:
    """radiance as the tests hold it: table [nodes, levels, R * R, 4] in the nodes' order and the levels' alphas"""

    def __init__(self, table, alphas):
        self.table = np.ascontiguousarray(table, F)
        self.alphas = [F(a) for a in alphas]
        self.res = int(round(np.sqrt(self.table.shape[2])))
        assert self.table.shape[1:] == (len(self.alphas), self.res * self.res, 4)

    def set_on(self, r):
        r.set_probe_grid_radiance(self.table, [float(a) for a in self.alphas])


def random_radiance(g, R, alphas, seed):
    """a seeded table in [0, 5): every node's, the invalid ones' included (the setter keeps those as zeros and the lookup never reads them)"""
    rng = np.random.default_rng(seed)
    nodes = g.count[0] * g.count[1] * g.count[2]
    t = rng.uniform(0.0, 5.0, (nodes, len(alphas), R * R, 4)).astype(F)
    t[..., 3] = 0.0
    return Radiance(t, alphas)


def reflect(d, n):
    """reflect_rs: d - (2 * dot(n, d)) * n"""
    dot = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    return (d - (F(2.0) * dot)[:, None] * n).astype(F)


def level_of(rad, a):
    """(l, l', t) of THE SPECULAR LOOKUP for alphas a [k]"""
    al = rad.alphas
    a = np.asarray(a, F).copy()
    a = np.where(~(a > al[0]), al[0], a).astype(F)
    l = np.zeros(a.shape[0], np.int64)
    for k in range(1, len(al)):
        l = np.where(al[k] <= a, k, l)
    top = l + 1 >= len(al)
    l1 = np.where(top, l, l + 1)
    lo = np.array(al, F)[l]; hi = np.array(al, F)[l1]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(top, F(0.0), (a - lo) / (hi - lo)).astype(F)
    return l, l1, t


def specular(g, depth, rad, P, n, d, a):
    """THE SPECULAR LOOKUP of include/pt_api.h at positions P, normals n, incoming directions d [k, 3] and alphas a [k]; depth None: the
    plain corner weights -> (S / W [k, 3] float32, lit [k] uint8)"""
    P = np.asarray(P, F).reshape(-1, 3); n = np.asarray(n, F).reshape(-1, 3); d = np.asarray(d, F).reshape(-1, 3)
    k = P.shape[0]
    a = np.broadcast_to(np.asarray(a, F), (k,))
    one = F(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pp = [(P[:, ax] + g.bias * n[:, ax]).astype(F) for ax in range(3)]
        i0, i1, f = [], [], []
        for ax in range(3):
            x = (pp[ax] - g.origin[ax]) / g.cell[ax]
            top = F(g.count[ax] - 1)
            x = np.where(~(x > F(0.0)), F(0.0), np.where(x > top, top, x)).astype(F)
            lo = np.trunc(x).astype(np.int64)
            i0.append(lo); i1.append(np.where(lo + 1 < g.count[ax], lo + 1, lo)); f.append((x - np.trunc(x)).astype(F))
        texel = PD.oct_texel(reflect(d, n), rad.res)
        l, l1, t = level_of(rad, a)
        t1 = one - t
        W = np.zeros(k, F); S = np.zeros((k, 3), F)
        for c in range(8):
            idx = [i1[ax] if c & (1 << ax) else i0[ax] for ax in range(3)]
            wx = f[0] if c & 1 else one - f[0]; wy = f[1] if c & 2 else one - f[1]; wz = f[2] if c & 4 else one - f[2]
            w = ((wx * wy) * wz) * np.where(g.valid[idx[2], idx[1], idx[0]], one, F(0.0)).astype(F)
            node = (idx[2] * g.count[1] + idx[1]) * g.count[0] + idx[0]
            if depth is not None:
                v = [(pp[ax] - (g.origin[ax] + idx[ax].astype(F) * g.cell[ax])).astype(F) for ax in range(3)]
                r = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
                m = depth.moments[node, PD.oct_texel(np.stack(v, axis=1), depth.res)]
                m1, m2 = m[:, 0], m[:, 1]
                var = np.abs(m2 - m1 * m1); dl = r - m1
                ch = var / (var + dl * dl); c3 = (ch * ch) * ch
                w = w * np.where(r > m1, np.where(c3 > depth.vis_floor, c3, depth.vis_floor), one).astype(F)
                if depth.facing:
                    cs = ((v[0] * n[:, 0] + v[1] * n[:, 1]) + v[2] * n[:, 2]) / r
                    hh = (one - cs) * F(0.5)
                    w = w * np.where(r > F(0.0), hh * hh + F(0.2), one).astype(F)
            T0 = rad.table[node, l, texel, :3]; T1 = rad.table[node, l1, texel, :3]
            T0 = np.where(g.valid[idx[2], idx[1], idx[0]][:, None], T0, F(0.0)).astype(F)    # the setter keeps an invalid node as zeros
            T1 = np.where(g.valid[idx[2], idx[1], idx[0]][:, None], T1, F(0.0)).astype(F)
            Lk = t1[:, None] * T0 + t[:, None] * T1
            S = S + w[:, None] * Lk
            W = W + w
            assert W.dtype == F and S.dtype == F and Lk.dtype == F
        lit = W > F(0.0)
        out = np.where(lit[:, None], S / W[:, None], F(0.0)).astype(F)
    return out, lit.astype(np.uint8)


def query(g, k, seed):
    """probe_grid_common.query_points with an incoming direction and an alpha for each: unit directions, and alphas that straddle [0, 1.2]"""
    P, n = PG.query_points(g, k, seed)
    d = PG.unit_normals(P.shape[0], seed + 2)
    a = np.random.default_rng(seed + 3).uniform(0.0, 1.2, P.shape[0]).astype(F)
    return P, n, d, a


# ------------------------------------------------------------------------------------------------------------------------------ the chain
def metal_alpha(roughness):
    """the GGX alpha of a material: roughness squared, clamped to [0.0001, 0.9999] (GGX::new_metal)"""
    a = F(roughness) * F(roughness)
    return F(0.0001) if a < F(0.0001) else (F(0.9999) if a > F(0.9999) else a)


def baked(orc, desc, maps, grid, depth, rad, o, d, max_hops, unlit=(0.0, 0.0, 0.0)):
    """probe_depth_common.baked with the metal ending: a chain that ends on GGX metal, on either face, is B = R * S where the specular lookup
    is lit, before any map is asked; everything else is the probe ending's.  rad None: the same walk without the metal ending, which is
    probe_depth_common.baked's (the tests hold the two to each other).
    Returns B [n, 3], how every chain ended [n] (PG.LIGHT .. METAL_BACK) and whether its last surface is GGX metal [n] (false for a miss)."""
    o = np.asarray(o, F).reshape(-1, 3).copy(); d = np.asarray(d, F).reshape(-1, 3).copy()
    n = o.shape[0]
    unlit = np.asarray(unlit, F)
    leaf_model = world_instance_models(desc)
    B = np.zeros((n, 3), F); ending = np.full(n, -1, np.int64); on_metal = np.zeros(n, bool)
    live = np.arange(n)
    prod = None
    for h in range(max_hops + 1):
        if live.size == 0:
            break
        tc = orc.trace_closest(o, d)
        hit = tc["inst"] != MISS
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
        c = scene_surface_colour(desc, leaf_model, inst, prim, u, v)
        if h:
            c = prod * c
        model = leaf_model[inst]
        wo = np.zeros_like(d); go = np.zeros(len(live), bool); light = np.zeros(len(live), bool)
        metal = np.zeros(len(live), bool); alpha = np.zeros(len(live), F)
        for mi in np.unique(model):
            sel = model == mi
            mat = desc.models[int(mi)].material
            w, followed, _ = G.follow_dir(mat.kind, mat.ior, d[sel], nrm[sel], front[sel])
            wo[sel] = w; go[sel] = followed & (h < max_hops)
            light[sel] = mat.kind == EMISSIVE
            metal[sel] = mat.kind == GGX_METAL
            alpha[sel] = metal_alpha(mat.roughness)
        e = ~go
        lm, mapped = BC.scene_lookup(desc, maps, inst[e], prim[e], u[e], v[e])
        mapped = mapped.astype(bool)
        usable = mapped & front[e]
        irr, lit = PD.lookup(grid, depth, p[e], nrm[e])
        lit = lit.astype(bool)
        if rad is None:
            spec, slit = np.zeros((int(e.sum()), 3), F), np.zeros(int(e.sum()), bool)
        else:
            spec, slit = specular(grid, depth, rad, p[e], nrm[e], d[e], alpha[e])
        shiny = metal[e] & slit.astype(bool)
        on_metal[live[e]] = metal[e]
        factor = np.where(usable[:, None], lm, np.where(lit[:, None], irr, unlit[None, :])).astype(F)
        factor = np.where(shiny[:, None], spec, factor).astype(F)
        b = np.where(light[e][:, None], c[e], c[e] * factor).astype(F)
        B[live[e]] = b
        other = np.where(mapped, np.where(lit, PG.PROBE_BACK, PG.UNLIT_BACK), np.where(lit, PG.PROBE_UNMAPPED, PG.UNLIT_UNMAPPED))
        kind = np.where(light[e], PG.LIGHT, np.where(usable, PG.MAPPED_FRONT, other))
        ending[live[e]] = np.where(shiny, np.where(front[e], METAL_FRONT, METAL_BACK), kind)
        live, o, d, prod = live[go], p[go], wo[go], c[go]
    assert (ending >= 0).all() and B.dtype == F
    return B, ending, on_metal


# ------------------------------------------------------------------------------- what prefiltered probes cost on a metal box in the Cornell box
# The end-to-end test of tests/test_gpu_probe_radiance.py compares the mean luminance of the baked view with pt_render's over the pixels whose
# chain ends on the metal: cornell_models(tall_material=E2E_METAL), probe_grid_common's 4 x 4 x 4 grid, R = 8, bake_probe_grid's five levels.
# Its bound is twice RADIANCE_FIGURE, derived below on the CPU from oracle pieces alone (PYTHONPATH=. python tests/probe_radiance_common.py
# prints it; nothing of the library's device code takes part):
#   * the grid and the radiance table are baked by the oracle: pt_probe_ray's directions (host evaluation), Oracle.integrate from every node,
#     the SH sums as probe_grid_common.oracle_probe_grid folds them, the radiance maps through the restated fold and the restated prefilter;
#   * the metal points are the first hits of the view's own camera rays (sample 0 of every pixel of the E2E frame) on the tall box;
#   * at each of them a_i = l(R_i * specular(grid, table, P_i, n_i, d_i, alpha)) is what the view shows and b_i = l(mean over E2E_PATHS
#     samples of Oracle.integrate along the camera ray itself) what it should show: the path's first bounce draws the material's own
#     direction and carries its own weight, and next-event estimation adds the lamp's highlight;
#   * the points are grouped by the face they lie on (the hit's normal), and RADIANCE_FIGURE = sum over faces |sum_f a - sum_f b| / sum b.
# What goes into the figure: the split-sum assumption V = N = R (the lobe of a metal seen at an angle is stretched and shifted off the mirror
# direction, the prefilter's is round and centred on it); nearest texels of an 8 x 8 map and nearest level pairs; the grid's trilinear blend of
# probes that stand up to a cell away from the surface, with no parallax correction; and the G term with the material's own weight, which a
# path loses energy to and R_H * S does not.  Grouping is section 24's: noise averages out within a face, nothing cancels between faces.
E2E_METAL_COLOUR, E2E_METAL_ROUGHNESS, E2E_RES, E2E_ALPHAS, E2E_PATHS = (0.9, 0.8, 0.6), 0.4, 8, (0.1, 0.2, 0.4, 0.7, 1.0), 4096
RADIANCE_FIGURE = 0.1469   # as derived with the parameters above: 61 of 64 nodes valid, 43 metal points on two faces of the tall box; shown against
#                            path traced +11.1 % on the face towards the camera (40 points), -63.0 % on the side face seen at a grazing angle
#                            (3 points), the sums +6.0 %
DIFFUSE_FIGURE = 0.9070    # the same statistic for the view without radiance (the metal shaded as a diffuse surface from the SH9 probes):
#                            +93.5 % and -53.5 %, the sums +83.3 %: it misses twice RADIANCE_FIGURE by a factor of three


def e2e_scene(w=PG.E2E_W, h=PG.E2E_H):
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import GGX, SceneDesc
    metal = GGX.new_metal(E2E_METAL_COLOUR, E2E_METAL_ROUGHNESS)
    return SceneDesc.new(scenes.cornell_models(tall_material=metal), scenes.reference_camera(w / h), "cornell, metal tall box")


def metal_pixels(orc, desc, w=PG.E2E_W, h=PG.E2E_H):
    """(pixel indices, o, d, the oracle's hits) of sample 0's camera rays whose first hit is GGX metal"""
    o, d = G.pinhole_rays(orc, w, h, 0)
    tc = orc.trace_closest(o, d)
    leaf_model = world_instance_models(desc)
    hit = tc["inst"] != MISS
    model = np.where(hit, leaf_model[np.where(hit, tc["inst"], 0)], -1)
    idx = np.nonzero(np.array([mi >= 0 and desc.models[int(mi)].material.kind == GGX_METAL for mi in model]))[0]
    return idx, o, d, tc


def radiance_figure(orc, r, desc, paths=E2E_PATHS):
    """the derivation above: ({"radiance": (figure, signed, groups), "diffuse": (...)}, valid nodes, {"radiance": one standard error of the
    figure from the paths' own scatter, "diffuse": ...}), groups {face normal: (points, sum a, sum b)}; "diffuse" is the same statistic for
    what the view shows without radiance, R_i * the SH9 lookup"""
    grid = PG.oracle_probe_grid(orc, r, desc)
    pos = grid.nodes().reshape(-1, 3)
    dirs, L = oracle_rays(orc, r, pos, PG.E2E_PROBE_SPP, PG.E2E_BOUNCES)
    rad = Radiance(prefilter(*fold_rays(dirs, L, E2E_RES), E2E_ALPHAS), E2E_ALPHAS)
    idx, o, d, tc = metal_pixels(orc, desc)
    P = G.fma32(d[idx], tc["t"][idx][:, None], o[idx]); nrm = tc["normal"][idx]
    leaf_model = world_instance_models(desc)
    R = scene_surface_colour(desc, leaf_model, tc["inst"][idx], tc["prim"][idx], tc["u"][idx], tc["v"][idx]).astype(np.float64)
    alpha = metal_alpha(E2E_METAL_ROUGHNESS)
    shown = {"radiance": BC.luminance(R * specular(grid, None, rad, P, nrm, d[idx], alpha)[0]), "diffuse": BC.luminance(R * PG.lookup(grid, P, nrm)[0])}
    b = np.zeros(len(idx)); se = np.zeros(len(idx))
    for i, px in enumerate(idx):
        paths_rgb = np.array([orc.integrate(o[px], d[px], int(px), s, 1, max_bounces=PG.E2E_BOUNCES + 1)[0][:3] for s in range(paths)], np.float64)
        lum = BC.luminance(paths_rgb)
        b[i], se[i] = lum.mean(), lum.std(ddof=1) / np.sqrt(paths)
    face = [tuple(np.round(n.astype(np.float64), 2).tolist()) for n in nrm]
    out = {}
    for name, a in shown.items():
        groups = {}
        for f in sorted(set(face)):
            sel = np.array([g == f for g in face])
            groups[f] = (int(sel.sum()), float(a[sel].sum()), float(b[sel].sum()))
        out[name] = (float(sum(abs(ga - gb) for _, ga, gb in groups.values()) / b.sum()), float((a.sum() - b.sum()) / b.sum()), groups)
    # the figure's own noise: a face's sum of b has the root of its points' squared standard errors, each face's term moves by that over
    # sum b, and the denominator's own error moves the whole figure by its relative size (first order, the faces' errors added, not squared)
    sigma = {name: float((sum(np.sqrt((se[np.array([g == f for g in face])] ** 2).sum()) for f in set(face)) + fig * np.sqrt((se ** 2).sum())) / b.sum())
             for name, (fig, _, _) in out.items()}
    return out, int(grid.valid.sum()), sigma


if __name__ == "__main__":          # the derivation of RADIANCE_FIGURE: CPU only, about a minute
    import time
    from oracle import oracle as O
    from path_tracer_amd import api
    O.build()
    t0 = time.time()
    sc = e2e_scene()
    res, n_valid, sigma = radiance_figure(O.Oracle(sc), api.Renderer(sc, PG.E2E_W, PG.E2E_H), sc)
    print(f"oracle-baked grid and radiance table: {n_valid} of 64 nodes valid ({time.time() - t0:.0f} s); one standard error of the figures: {sigma}")
    for name, (figure, signed, groups) in res.items():
        for f, (k, ga, gb) in groups.items():
            print(f"  {name:9s} face {f}: {k:4d} points: shown {ga / k:.5f}, path traced {gb / k:.5f}, {(ga - gb) / gb:+.4f}")
        print(f"{name}: figure = {figure:.4f} (signed difference of the sums {signed:+.4f}); twice it is {2 * figure:.4f}")
