"""Shared by tests/test_probe_grid_host.py and tests/test_gpu_probe_grid.py: the probe grid's lookup of include/pt_api.h (pt_set_probe_grid)
restated in numpy, every product, sum, difference and quotient ONE np.float32 operation in the order the header writes them; the baked
sample with the probe ending, over baked_common's oracle-walked chain; the census of probes inside geometry over the oracle's trace_closest;
and the grids the tests set.  Nothing here calls the library's device code."""
import numpy as np

import baked_common as BC
import guides_follow_common as G
from path_tracer_amd.scene_desc import EMISSIVE
from textures_common import scene_surface_colour, world_instance_models

F = np.float32
MISS = 0xFFFFFFFF
COSINE = (F(1.0), F(0.6666667), F(0.25))          # the cosine lobe over pi, per band
COUNTS = [(1, 1, 1), (2, 2, 2), (3, 2, 4), (5, 1, 3)]
# how a chain of the baked view ended, with a grid set (the table of pt_render_baked and its change under pt_set_probe_grid)
LIGHT, MAPPED_FRONT, PROBE_BACK, PROBE_UNMAPPED, UNLIT_BACK, UNLIT_UNMAPPED, MISS_AT_0, MISS_AFTER_HOPS = range(8)
ENDINGS = {LIGHT: "light", MAPPED_FRONT: "mapped front", PROBE_BACK: "probe-lit back face", PROBE_UNMAPPED: "probe-lit unmapped",
           UNLIT_BACK: "unlit back face", UNLIT_UNMAPPED: "unlit unmapped", MISS_AT_0: "miss at once", MISS_AFTER_HOPS: "miss after a hop"}


class Grid:
    """a grid as the tests hold it: count = (nx, ny, nz), sh [nz, ny, nx, 9, 3] radiance coefficients, valid [nz, ny, nx] bool"""

    def __init__(self, origin, cell, count, sh, valid=None, bias=0.0):
        self.origin = np.asarray(origin, F); self.cell = np.asarray(cell, F); self.count = tuple(int(k) for k in count)
        nx, ny, nz = self.count
        self.sh = np.asarray(sh, F).reshape(nz, ny, nx, 9, 3)
        self.valid = np.ones((nz, ny, nx), bool) if valid is None else np.asarray(valid).astype(bool).reshape(nz, ny, nx)
        self.bias = F(bias)

    def set_on(self, r):
        r.set_probe_grid(self.origin, self.cell, self.sh, self.valid, self.bias)

    def nodes(self):
        """the node positions [nz, ny, nx, 3]: origin + index * cell in binary32"""
        nx, ny, nz = self.count
        idx = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")[::-1], axis=-1).astype(F)
        return (self.origin + idx * self.cell).astype(F)


def random_grid(count, seed, invalid=0.0, bias=0.0, origin=(-1.0, 0.5, 2.0), cell=(0.5, 2.0, 0.25)):
    """seeded coefficients in [-1, 3), negative ones included; the default origin and cell are dyadic, so that node positions and the grid
    coordinates of nodes are exact"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = count
    sh = rng.uniform(-1.0, 3.0, (nz, ny, nx, 9, 3)).astype(F)
    valid = rng.uniform(0.0, 1.0, (nz, ny, nx)) >= invalid
    return Grid(origin, cell, count, sh, valid, bias)


# ---------------------------------------------------------------------------------------------------------------------------- the lookup
def sh9(n):
    """y0..y8 of directions n [k, 3] as pt_bake_probes states them -> [k, 9]"""
    n = np.asarray(n, F)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    out = np.empty((n.shape[0], 9), F)
    out[:, 0] = F(0.2820948)
    out[:, 1] = F(0.48860252) * y
    out[:, 2] = F(0.48860252) * z
    out[:, 3] = F(0.48860252) * x
    out[:, 4] = F(1.0925484) * (x * y)
    out[:, 5] = F(1.0925484) * (y * z)
    out[:, 6] = F(0.31539157) * (F(3.0) * (z * z) - F(1.0))
    out[:, 7] = F(1.0925484) * (x * z)
    out[:, 8] = F(0.54627424) * (x * x - y * y)
    return out


def lookup(g, P, n):
    """THE LOOKUP of include/pt_api.h at positions P and normals n [k, 3] -> (I [k, 3] float32, lit [k] uint8)"""
    P = np.asarray(P, F).reshape(-1, 3); n = np.asarray(n, F).reshape(-1, 3)
    k = P.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        i0, i1, f = [], [], []
        for a in range(3):
            x = ((P[:, a] + g.bias * n[:, a]) - g.origin[a]) / g.cell[a]
            top = F(g.count[a] - 1)
            x = np.where(~(x > F(0.0)), F(0.0), np.where(x > top, top, x)).astype(F)
            lo = np.trunc(x).astype(np.int64)
            i0.append(lo); i1.append(np.where(lo + 1 < g.count[a], lo + 1, lo)); f.append((x - np.trunc(x)).astype(F))
        yc = sh9(n)
        yc[:, 1:4] = COSINE[1] * yc[:, 1:4]
        yc[:, 4:9] = COSINE[2] * yc[:, 4:9]
        one = F(1.0)
        W = None; E = None
        for c in range(8):
            ix = i1[0] if c & 1 else i0[0]; iy = i1[1] if c & 2 else i0[1]; iz = i1[2] if c & 4 else i0[2]
            wx = f[0] if c & 1 else one - f[0]; wy = f[1] if c & 2 else one - f[1]; wz = f[2] if c & 4 else one - f[2]
            w = ((wx * wy) * wz) * np.where(g.valid[iz, iy, ix], one, F(0.0)).astype(F)
            L = g.sh[iz, iy, ix]                                               # [k, 9, 3]
            e = yc[:, 0, None] * L[:, 0] + yc[:, 1, None] * L[:, 1]
            for m in range(2, 9):
                e = e + yc[:, m, None] * L[:, m]
            we = w[:, None] * e
            W = w if W is None else W + w
            E = we if E is None else E + we
        assert W.dtype == F and E.dtype == F
        lit = W > F(0.0)
        I = E / W[:, None]
        I = np.where(lit[:, None] & (I > F(0.0)), I, F(0.0)).astype(F)
    assert I.shape == (k, 3)
    return I, lit.astype(np.uint8)


def node_evaluation(g, n):
    """e of every node for the one normal n [3]: [nz, ny, nx, 3], the header's corner evaluation"""
    yc = sh9(np.asarray(n, F).reshape(1, 3))[0]
    yc[1:4] = COSINE[1] * yc[1:4]
    yc[4:9] = COSINE[2] * yc[4:9]
    e = yc[0] * g.sh[..., 0, :] + yc[1] * g.sh[..., 1, :]
    for m in range(2, 9):
        e = e + yc[m] * g.sh[..., m, :]
    assert e.dtype == F
    return e


def unit_normals(k, seed):
    v = np.random.default_rng(seed).normal(size=(k, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def query_points(g, k, seed):
    """k random points inside the grid's box, then every node position, points beyond each face and corner, huge and NaN ones; and a unit
    normal for each"""
    rng = np.random.default_rng(seed)
    span = g.cell * (np.asarray(g.count, F) - F(1.0))
    inside = (g.origin + rng.uniform(0.0, 1.0, (k, 3)).astype(F) * span).astype(F)
    outside = []
    for sx in (-1.5, 0.5, 2.5):
        for sy in (-1.5, 0.5, 2.5):
            for sz in (-1.5, 0.5, 2.5):
                outside.append(g.origin + np.array([sx, sy, sz], F) * np.maximum(span, g.cell))
    odd = np.array([[np.nan, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, np.nan], [np.nan] * 3, [1e30, 1e30, 1e30], [-1e30, 1e30, 0.0],
                    [1e30, -1e30, -1e30], [np.inf, -np.inf, 0.0]], F)
    P = np.concatenate([inside, g.nodes().reshape(-1, 3), np.array(outside, F), odd]).astype(F)
    return P, unit_normals(P.shape[0], seed + 1)


def constant_radiance_sh(c):
    """the SH9 projection of the constant radiance c [3]: L_0 = c * sqrt(4 pi), every other coefficient 0 -> [9, 3]"""
    sh = np.zeros((9, 3), F)
    sh[0] = np.asarray(c, np.float64) * np.sqrt(4.0 * np.pi)
    return sh


# ------------------------------------------------------------------------------------------------------------------------------ the chain
def baked(orc, desc, maps, grid, o, d, max_hops, unlit=(0.0, 0.0, 0.0)):
    """baked_common.baked with the probe ending: B [n, 3] of rays (o, d) followed through `desc`, and how every chain ended [n]
    (LIGHT .. MISS_AFTER_HOPS).  grid None: the view without a grid (the unlit endings only)."""
    o = np.asarray(o, F).reshape(-1, 3).copy(); d = np.asarray(d, F).reshape(-1, 3).copy()
    n = o.shape[0]
    unlit = np.asarray(unlit, F)
    leaf_model = world_instance_models(desc)
    B = np.zeros((n, 3), F); ending = np.full(n, -1, np.int64)
    live = np.arange(n)
    prod = None
    for h in range(max_hops + 1):
        if live.size == 0:
            break
        tc = orc.trace_closest(o, d)
        hit = tc["inst"] != MISS
        miss = live[~hit]
        B[miss] = BC.AMBIENT if prod is None else prod[~hit] * BC.AMBIENT
        ending[miss] = MISS_AFTER_HOPS if h else MISS_AT_0
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
        for mi in np.unique(model):
            sel = model == mi
            mat = desc.models[int(mi)].material
            w, followed, _ = G.follow_dir(mat.kind, mat.ior, d[sel], nrm[sel], front[sel])
            wo[sel] = w; go[sel] = followed & (h < max_hops)
            light[sel] = mat.kind == EMISSIVE
        e = ~go
        lm, mapped = BC.scene_lookup(desc, maps, inst[e], prim[e], u[e], v[e])
        mapped = mapped.astype(bool)
        usable = mapped & front[e]
        if grid is None:
            irr, lit = np.zeros((int(e.sum()), 3), F), np.zeros(int(e.sum()), bool)
        else:
            irr, lit = lookup(grid, p[e], nrm[e])
            lit = lit.astype(bool)
        factor = np.where(usable[:, None], lm, np.where(lit[:, None], irr, unlit[None, :])).astype(F)
        b = np.where(light[e][:, None], c[e], c[e] * factor).astype(F)
        B[live[e]] = b
        other = np.where(mapped, np.where(lit, PROBE_BACK, UNLIT_BACK), np.where(lit, PROBE_UNMAPPED, UNLIT_UNMAPPED))
        ending[live[e]] = np.where(light[e], LIGHT, np.where(usable, MAPPED_FRONT, other))
        live, o, d, prod = live[go], p[go], wo[go], c[go]
    assert (ending >= 0).all() and B.dtype == F
    return B, ending


# ----------------------------------------------------------------------------------------------------------------------------- the census
def census(orc, r, positions, n_samples, first_sample=0, key_base=0):
    """(hits [n], back [n]) of pt_probe_backfaces: the directions are pt_probe_ray's (host evaluation, held to its definition by
    tests/test_gpu_rays.py), every ray traced once by the oracle, the front flag the one the guides use"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    hits = np.zeros(pos.shape[0], np.uint32); back = np.zeros(pos.shape[0], np.uint32)
    for j in range(pos.shape[0]):
        d = np.array([r.probe_ray(key_base + j, first_sample + s)[0] for s in range(n_samples)], F)
        tc = orc.trace_closest(np.repeat(pos[j][None], n_samples, axis=0), d)
        hit = tc["inst"] != MISS
        hits[j] = hit.sum()
        back[j] = (hit & (tc["front"] == 0)).sum()
    return hits, back


# ------------------------------------------------------------------------------------------------- what SH9 probes cost in the Cornell box
# The end-to-end test of tests/test_gpu_probe_grid.py compares the frame-mean luminance of the probe-lit baked view with pt_render's.  Its
# bound is twice SH9_FIGURE, the error that band-2 probes on a 4 x 4 x 4 grid make on THIS scene, derived below on the CPU from oracle
# pieces alone (PYTHONPATH=. python tests/probe_grid_common.py prints it; nothing of the library's device code takes part):
#   * the grid of cornell_grid() is baked by the oracle: pt_probe_ray's directions (host evaluation), Oracle.integrate from every node,
#     folded in float64, times 4 pi / n; a node is valid under Renderer.probe_validity's rule over Oracle.trace_closest's front flag;
#   * the wall points are the first hits of the view's own camera rays (sample 0 of every pixel of the E2E frame) on anything but the light;
#   * at each of them a_i = l(R_i * lookup(grid, P_i, n_i)) is what the view shows and b_i = l(R_i * mean of Oracle.integrate over E2E_COSINE
#     cosine-distributed directions from P_i) what it should show (irradiance over pi, the lightmap's unit; R_i the surface colour);
#   * the points are grouped by the model they lie on (floor, ceiling and back wall are one model; each side wall and each box another), and
#     SH9_FIGURE = sum over groups |sum_g a - sum_g b| / sum over all points b.
# Grouping is what keeps the figure honest in both directions: within a group the Monte Carlo noise of b (a cosine ray meets the small light
# with a probability of a few per cent) averages out over some 10^5 rays instead of being counted as error point by point, and between
# groups nothing cancels, so by the triangle inequality the figure is at least the relative difference of the two frame sums, which is the
# statistic the GPU test measures (there over a frame that also holds light and miss pixels, equal on both sides: a larger denominator).
E2E_W, E2E_H, E2E_BOUNCES, E2E_COUNT, E2E_PROBE_SPP, E2E_COSINE = 48, 32, 3, (4, 4, 4), 1024, 2048
SH9_FIGURE = 0.1641   # as derived with the parameters above: 61 of 64 nodes valid, 447 wall points; per model SH9 against cosine-sampled
#                       cb_main +16.8 %, cb_right +23.5 %, cb_left -1.2 %, cb_box_tall +40.0 %, cb_box_short -13.6 %, the sums +14.9 %
#                       (with 512 cosine rays a point instead of 2 048 the figure is 0.1495: what is left of the reference's own noise)


def cornell_grid(desc, count=E2E_COUNT):
    """(origin, cell) of a grid over the bounds of desc's vertices, inset by half a cell (examples/headless --probe-grid's placement)"""
    p = np.concatenate([np.asarray(m.positions, F).reshape(-1, 3) for m in desc.models])
    lo, hi = p.min(0), p.max(0)
    cell = ((hi - lo) / np.asarray(count, F)).astype(F)
    return (lo + F(0.5) * cell).astype(F), cell


def oracle_probe_grid(orc, r, desc, n_samples=E2E_PROBE_SPP, depth=E2E_BOUNCES, count=E2E_COUNT, max_back_fraction=0.25):
    """bake_probe_grid by the oracle: a Grid of radiance coefficients (sums * 4 pi / n, float64 sums) with probe_validity's rule.  r gives
    pt_probe_ray (host evaluation) and nothing else."""
    origin, cell = cornell_grid(desc, count)
    g = Grid(origin, cell, count, np.zeros(count[::-1] + (9, 3), F))
    pos = g.nodes().reshape(-1, 3)
    sh = np.zeros((pos.shape[0], 9, 3)); valid = np.zeros(pos.shape[0], bool)
    for j in range(pos.shape[0]):
        rays = [r.probe_ray(j, s) for s in range(n_samples)]
        d = np.array([q[0] for q in rays], F); y = np.array([q[1] for q in rays], np.float64)
        rad = np.array([orc.integrate(pos[j], d[s], j, s, 1, max_bounces=depth)[0][:3] for s in range(n_samples)], np.float64)
        sh[j] = y.T @ rad
        tc = orc.trace_closest(np.repeat(pos[j][None], n_samples, axis=0), d)
        back = ((tc["inst"] != MISS) & (tc["front"] == 0)).sum()
        valid[j] = back <= max_back_fraction * n_samples
    return Grid(origin, cell, count, (sh * (4.0 * np.pi / n_samples)).astype(F), valid)


def _cosine_directions(n, k, rng):
    """k cosine-distributed unit directions about the unit normal n [3], float64"""
    u1, u2 = rng.uniform(size=k), rng.uniform(size=k)
    rr, phi = np.sqrt(u1), 2.0 * np.pi * u2
    a = np.array([0.0, 1.0, 0.0]) if abs(n[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    t = np.cross(n, a); t /= np.linalg.norm(t)
    b = np.cross(n, t)
    return (rr * np.cos(phi))[:, None] * t + (rr * np.sin(phi))[:, None] * b + np.sqrt(1.0 - u1)[:, None] * n


def sh9_figure(orc, desc, grid, w=E2E_W, h=E2E_H, depth=E2E_BOUNCES, n_cosine=E2E_COSINE, seed=61):
    """the derivation above: (figure, signed relative difference of the sums, {model name: (points, sum a, sum b)})"""
    o, d = G.pinhole_rays(orc, w, h, 0)
    tc = orc.trace_closest(o, d)
    leaf_model = world_instance_models(desc)
    hit = tc["inst"] != MISS
    model = np.where(hit, leaf_model[np.where(hit, tc["inst"], 0)], -1)
    wall = hit & np.array([mi >= 0 and desc.models[int(mi)].material.kind != EMISSIVE for mi in model])
    idx = np.nonzero(wall)[0]
    P = G.fma32(d[idx], tc["t"][idx][:, None], o[idx]); nrm = tc["normal"][idx]
    R = scene_surface_colour(desc, leaf_model, tc["inst"][idx], tc["prim"][idx], tc["u"][idx], tc["v"][idx]).astype(np.float64)
    a = BC.luminance(R * lookup(grid, P, nrm)[0])
    rng = np.random.default_rng(seed)
    reach = float(np.abs(grid.cell).max())
    b = np.zeros(len(idx))
    for i in range(len(idx)):
        nn = nrm[i].astype(np.float64)
        dirs = _cosine_directions(nn / np.linalg.norm(nn), n_cosine, rng).astype(F)
        start = (P[i] + F(1e-4 * reach) * nrm[i]).astype(F)
        rad = np.array([orc.integrate(start, dirs[s], int(idx[i]), s, 1, max_bounces=depth)[0][:3] for s in range(n_cosine)], np.float64)
        b[i] = BC.luminance(R[i] * rad.mean(0))
    groups = {}
    for mi in np.unique(model[idx]):
        sel = model[idx] == mi
        groups[desc.models[int(mi)].name] = (int(sel.sum()), float(a[sel].sum()), float(b[sel].sum()))
    figure = sum(abs(ga - gb) for _, ga, gb in groups.values()) / b.sum()
    return float(figure), float((a.sum() - b.sum()) / b.sum()), groups


# ------------------------------------------------------------------------------------------------------------------------------ the room
def room_grid(seed=31):
    """a 3 x 2 x 4 grid inside baked_common.mapped_room with seeded positive coefficients (band 0 dominant, so that most evaluations are
    positive) and two invalid nodes, (0, 0, 0) and (0, 1, 0): every point beyond both the x-min and the z-min face blends those two alone,
    and there the grid is not lit"""
    rng = np.random.default_rng(seed)
    sh = rng.uniform(-0.3, 0.3, (4, 2, 3, 9, 3)).astype(F)
    sh[..., 0, :] = rng.uniform(1.0, 3.0, (4, 2, 3, 3)).astype(F)
    valid = np.ones((4, 2, 3), bool)
    valid[0, 0, 0] = valid[0, 1, 0] = False
    return Grid((-2.0, -7.0, -10.0), (5.0, 9.0, 5.0), (3, 2, 4), sh, valid, bias=0.125)


if __name__ == "__main__":          # the derivation of SH9_FIGURE: CPU only, a few minutes
    import time
    from oracle import oracle as O
    from path_tracer_amd import api, scenes
    O.build()
    t0 = time.time()
    sc = scenes.cornell_box(E2E_W, E2E_H)
    orc = O.Oracle(sc)
    grid = oracle_probe_grid(orc, api.Renderer(sc, E2E_W, E2E_H), sc)
    print(f"oracle-baked grid: {int(grid.valid.sum())} of {grid.valid.size} nodes valid ({time.time() - t0:.0f} s)")
    figure, signed, groups = sh9_figure(orc, sc, grid)
    for name, (k, ga, gb) in groups.items():
        print(f"  {name:14s} {k:5d} points: SH9 {ga / k:.5f}, cosine-sampled {gb / k:.5f}, {(ga - gb) / gb:+.4f}")
    print(f"SH9_FIGURE = {figure:.4f} (signed difference of the sums {signed:+.4f}); the bound is {2 * figure:.4f} ({time.time() - t0:.0f} s)")
