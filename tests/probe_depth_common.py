"""Shared by tests/test_probe_depth_host.py and tests/test_gpu_probe_depth.py: probe visibility (include/pt_api.h, pt_set_probe_grid_depth)
restated in numpy, every product, sum, difference, quotient and square root ONE np.float32 operation in the order the header writes them: the
octahedral texel and its inverse, the depth bake's fold over the oracle's trace_closest, the means, the lookup with visibility on top of
probe_grid_common's grids, and the baked sample with that lookup over baked_common's oracle-walked chain.  Nothing here calls the library's
device code."""
import numpy as np

import baked_common as BC
import guides_follow_common as G
import probe_grid_common as PG
from path_tracer_amd.scene_desc import EMISSIVE
from textures_common import scene_surface_colour, world_instance_models

F = np.float32
MISS = PG.MISS
FACING = 1


# ------------------------------------------------------------------------------------------------------------------------------ the texel
def oct_texel(v, R):
    """THE TEXEL of include/pt_api.h for directions v [k, 3] (any values) in a map of side R -> [k] int64"""
    v = np.asarray(v, F).reshape(-1, 3)
    one, half, fr = F(1.0), F(0.5), F(R)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = (np.abs(v[:, 0]) + np.abs(v[:, 1])) + np.abs(v[:, 2])
        px, py = v[:, 0] / s, v[:, 1] / s
        qx = (one - np.abs(py)) * np.where(px >= F(0.0), one, -one).astype(F)
        qy = (one - np.abs(px)) * np.where(py >= F(0.0), one, -one).astype(F)
        neg = v[:, 2] < F(0.0)
        px, py = np.where(neg, qx, px).astype(F), np.where(neg, qy, py).astype(F)
        out = []
        for q in (px, py):
            ur = (q * half + half) * fr
            assert ur.dtype == F
            pos = ur > F(0.0)
            out.append(np.where(pos, np.minimum(np.trunc(np.where(pos, ur, F(0.0))).astype(np.int64), R - 1), 0))
    return out[1] * R + out[0]


def oct_centre_directions(R):
    """the numpy inverse: the unit direction through the centre of every texel of a map of side R, float64 -> [R * R, 3]"""
    iy, ix = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    px = (ix.reshape(-1) + 0.5) / R * 2.0 - 1.0
    py = (iy.reshape(-1) + 0.5) / R * 2.0 - 1.0
    z = 1.0 - np.abs(px) - np.abs(py)
    lower = z < 0
    x = np.where(lower, (1.0 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0), px)
    y = np.where(lower, (1.0 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0), py)
    d = np.stack([x, y, z], axis=1)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------------------- the bake
def fold(directions, t, hit, R, max_distance, sums, counts):
    """THE BAKE's fold of one probe's rays, in the order given (sample order): sums [R * R, 2] float32 and counts [R * R] uint32 in place"""
    far = F(max_distance)
    t = np.asarray(t, F)
    d = np.where(hit, np.where(t < far, t, far), far).astype(F)
    texel = oct_texel(directions, R)
    for s in range(len(d)):
        k = texel[s]
        counts[k] += 1
        sums[k, 0] = sums[k, 0] + d[s]
        sums[k, 1] = sums[k, 1] + d[s] * d[s]
    assert sums.dtype == F


def oracle_depth(orc, r, positions, n_samples, R, max_distance, first_sample=0, key_base=0, sums=None, counts=None):
    """pt_bake_probe_depth by the oracle: pt_probe_ray's directions (host evaluation), Oracle.trace_closest's t, the restated fold.
    orc None: the empty world, where every ray misses.  Returns (sums [n, R * R, 2], counts [n, R * R])."""
    pos = np.asarray(positions, F).reshape(-1, 3)
    sums = np.zeros((pos.shape[0], R * R, 2), F) if sums is None else np.array(sums, F).reshape(pos.shape[0], R * R, 2)
    counts = np.zeros((pos.shape[0], R * R), np.uint32) if counts is None else np.array(counts, np.uint32).reshape(pos.shape[0], R * R)
    for j in range(pos.shape[0]):
        d = np.array([r.probe_ray(key_base + j, first_sample + s)[0] for s in range(n_samples)], F)
        if orc is None:
            t, hit = np.zeros(n_samples, F), np.zeros(n_samples, bool)
        else:
            tc = orc.trace_closest(np.repeat(pos[j][None], n_samples, axis=0), d)
            t, hit = tc["t"], tc["inst"] != MISS
        fold(d, t, hit, R, max_distance, sums[j], counts[j])
    return sums, counts


def means(sums, counts, max_distance):
    """Renderer.set_probe_grid_depth_sums' division, one binary32 quotient each; a texel without a sample: (max_distance, max_distance^2)"""
    far = F(max_distance)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (np.asarray(sums, F) / np.asarray(counts).astype(F)[..., None]).astype(F)
    return np.where((np.asarray(counts) > 0)[..., None], m, np.array([far, far * far], F)).astype(F)


# ----------------------------------------------------------------------------------------------------------------------------- the lookup
class Depth:
    """depth as the tests hold it: moments [nodes, R * R, 2] in the nodes' order, the floor and the FACING flag"""

    def __init__(self, moments, vis_floor=0.0, facing=False):
        self.moments = np.ascontiguousarray(moments, F)
        self.res = int(round(np.sqrt(self.moments.shape[1])))
        assert self.moments.shape[1:] == (self.res * self.res, 2)
        self.vis_floor = F(vis_floor); self.facing = bool(facing)

    def set_on(self, r):
        r.set_probe_grid_depth(self.moments, float(self.vis_floor), self.facing)


def random_depth(g, R, seed, vis_floor=0.0, facing=False, consistent=True):
    """seeded moments of the size of g's cells: m2 >= m1^2 where consistent, m2 < m1^2 (the fabsf) where not"""
    rng = np.random.default_rng(seed)
    nodes = g.count[0] * g.count[1] * g.count[2]
    reach = float(np.linalg.norm(g.cell.astype(np.float64)))
    m1 = rng.uniform(0.05, 1.2, (nodes, R * R)).astype(F) * F(reach)
    spread = rng.uniform(0.0, 0.3, (nodes, R * R)).astype(F) * F(reach)
    m2 = (m1 * m1 + spread * spread).astype(F) if consistent else (m1 * m1 * rng.uniform(0.5, 0.99, m1.shape).astype(F)).astype(F)
    return Depth(np.stack([m1, m2], axis=-1), vis_floor, facing)


def far_depth(g, R):
    """every m1 beyond the grid's diagonal and the bias: nothing is occluded"""
    nodes = g.count[0] * g.count[1] * g.count[2]
    far = F(4.0) * F(np.linalg.norm((g.cell * np.asarray(g.count, F)).astype(np.float64)) + 1.0)
    return Depth(np.broadcast_to(np.array([far, far * far], F), (nodes, R * R, 2)).copy())


def lookup(g, depth, P, n):
    """THE LOOKUP WITH VISIBILITY of include/pt_api.h at positions P and normals n [k, 3] -> (I [k, 3] float32, lit [k] uint8); depth None:
    probe_grid_common.lookup"""
    if depth is None:
        return PG.lookup(g, P, n)
    P = np.asarray(P, F).reshape(-1, 3); n = np.asarray(n, F).reshape(-1, 3)
    k = P.shape[0]
    R = depth.res
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pp = [(P[:, a] + g.bias * n[:, a]).astype(F) for a in range(3)]
        i0, i1, f = [], [], []
        for a in range(3):
            x = (pp[a] - g.origin[a]) / g.cell[a]
            top = F(g.count[a] - 1)
            x = np.where(~(x > F(0.0)), F(0.0), np.where(x > top, top, x)).astype(F)
            lo = np.trunc(x).astype(np.int64)
            i0.append(lo); i1.append(np.where(lo + 1 < g.count[a], lo + 1, lo)); f.append((x - np.trunc(x)).astype(F))
        yc = PG.sh9(n)
        yc[:, 1:4] = PG.COSINE[1] * yc[:, 1:4]
        yc[:, 4:9] = PG.COSINE[2] * yc[:, 4:9]
        one = F(1.0)
        W = None; E = None
        for c in range(8):
            idx = [i1[a] if c & (1 << a) else i0[a] for a in range(3)]
            wx = f[0] if c & 1 else one - f[0]; wy = f[1] if c & 2 else one - f[1]; wz = f[2] if c & 4 else one - f[2]
            w = ((wx * wy) * wz) * np.where(g.valid[idx[2], idx[1], idx[0]], one, F(0.0)).astype(F)
            v = [(pp[a] - (g.origin[a] + idx[a].astype(F) * g.cell[a])).astype(F) for a in range(3)]
            r = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            node = (idx[2] * g.count[1] + idx[1]) * g.count[0] + idx[0]
            m = depth.moments[node, oct_texel(np.stack(v, axis=1), R)]
            m1, m2 = m[:, 0], m[:, 1]
            var = np.abs(m2 - m1 * m1); dl = r - m1
            ch = var / (var + dl * dl); c3 = (ch * ch) * ch
            vis = np.where(r > m1, np.where(c3 > depth.vis_floor, c3, depth.vis_floor), one).astype(F)
            w = w * vis
            if depth.facing:
                cs = ((v[0] * n[:, 0] + v[1] * n[:, 1]) + v[2] * n[:, 2]) / r
                h = (one - cs) * F(0.5)
                w = w * np.where(r > F(0.0), h * h + F(0.2), one).astype(F)
            assert r.dtype == F and w.dtype == F
            L = g.sh[idx[2], idx[1], idx[0]]                                   # [k, 9, 3]
            e = yc[:, 0, None] * L[:, 0] + yc[:, 1, None] * L[:, 1]
            for mm in range(2, 9):
                e = e + yc[:, mm, None] * L[:, mm]
            we = w[:, None] * e
            W = w if W is None else W + w
            E = we if E is None else E + we
        assert W.dtype == F and E.dtype == F
        lit = W > F(0.0)
        I = E / W[:, None]
        I = np.where(lit[:, None] & (I > F(0.0)), I, F(0.0)).astype(F)
    assert I.shape == (k, 3)
    return I, lit.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------ the chain
def baked(orc, desc, maps, grid, depth, o, d, max_hops, unlit=(0.0, 0.0, 0.0)):
    """probe_grid_common.baked with the lookup above in the probe ending: B [n, 3] and how every chain ended [n] (PG.LIGHT ..)"""
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
            irr, lit = lookup(grid, depth, p[e], nrm[e])
            lit = lit.astype(bool)
        factor = np.where(usable[:, None], lm, np.where(lit[:, None], irr, unlit[None, :])).astype(F)
        b = np.where(light[e][:, None], c[e], c[e] * factor).astype(F)
        B[live[e]] = b
        other = np.where(mapped, np.where(lit, PG.PROBE_BACK, PG.UNLIT_BACK), np.where(lit, PG.PROBE_UNMAPPED, PG.UNLIT_UNMAPPED))
        ending[live[e]] = np.where(light[e], PG.LIGHT, np.where(usable, PG.MAPPED_FRONT, other))
        live, o, d, prod = live[go], p[go], wo[go], c[go]
    assert (ending >= 0).all() and B.dtype == F
    return B, ending


# ------------------------------------------------------------------------------------------------------------------------------ two rooms
TWO_ROOMS_COUNT, TWO_ROOMS_SPP, TWO_ROOMS_BOUNCES, TWO_ROOMS_RES = (4, 2, 2), 256, 3, 8


def two_rooms_max_distance(cell):
    """bake_probe_grid's default: the cell's diagonal times 1.5"""
    return 1.5 * float(np.linalg.norm(np.asarray(cell, np.float64)))


def oracle_two_rooms(orc, r, desc):
    """scenes.two_rooms' 4 x 2 x 2 grid baked by the oracle (PG.oracle_probe_grid) and its depth (oracle_depth, R = 8) -> (Grid, Depth)"""
    grid = PG.oracle_probe_grid(orc, r, desc, n_samples=TWO_ROOMS_SPP, depth=TWO_ROOMS_BOUNCES, count=TWO_ROOMS_COUNT)
    far = two_rooms_max_distance(grid.cell)
    sums, counts = oracle_depth(orc, r, grid.nodes().reshape(-1, 3), TWO_ROOMS_SPP, TWO_ROOMS_RES, far)
    return grid, Depth(means(sums, counts, far))


def dark_room_points():
    """fixed points on the dark room's floor, back wall and partition with their normals; the first LEAK_POINTS lie in the cells that
    straddle the partition (0.125 < x < 2), the others beyond node column 2, where only dark-room nodes are blended"""
    xs_near, xs_far = (0.25, 0.75, 1.25, 1.75), (2.5, 4.0, 6.5)
    P, N = [], []
    for xs in (xs_near, xs_far):
        for x in xs:
            for z in (0.75, 2.0, 3.25):
                P.append((x, 0.0, z)); N.append((0.0, 1.0, 0.0))               # floor
            for y in (0.75, 2.0, 3.25):
                P.append((x, y, 0.0)); N.append((0.0, 0.0, 1.0))               # back wall
        if xs is xs_near:
            for y in (1.0, 3.0):
                for z in (1.0, 3.0):
                    P.append((0.125, y, z)); N.append((1.0, 0.0, 0.0))         # the partition's dark face
            n_near = len(P)
    return np.array(P, F), np.array(N, F), n_near


# ---------------------------------------------------------------------------------------- what SH9 probes with depth cost in the Cornell box
# The end-to-end test of tests/test_gpu_probe_depth.py is section 24's (probe_grid_common.SH9_FIGURE) with depth on the grid: R = 8, FACING
# on, vis_floor 0.  Its bound is twice DEPTH_FIGURE, which is probe_grid_common.sh9_figure run with the lookup above over an oracle-baked
# depth table (oracle_depth over the same 4 x 4 x 4 grid and the same 1 024 rays a node, max_distance = the cell's diagonal times 1.5): the
# same wall points, the same cosine-sampled truth, the same grouping by model.  PYTHONPATH=. python tests/probe_depth_common.py prints it.
E2E_RES, E2E_FLOOR, E2E_FACING = 8, 0.0, True
DEPTH_FIGURE = 0.1410   # as derived: 61 of 64 nodes valid, max_distance 361.13, 447 wall points; per model SH9 with depth against cosine-sampled
#                         cb_main +17.4 %, cb_right +22.4 %, cb_left -3.6 %, cb_box_tall +2.0 %, cb_box_short -5.5 %, the sums +12.5 %
#                         (the same run gives the plain lookup section 24's 0.1641 and +16.8, +23.5, -1.2, +40.0, -13.6 %)


def depth_figure(orc, desc, grid, depth):
    """PG.sh9_figure with the visibility lookup in place of the plain one"""
    plain = PG.lookup
    PG.lookup = lambda g, P, n: lookup(g, depth, P, n)
    try:
        return PG.sh9_figure(orc, desc, grid)
    finally:
        PG.lookup = plain


if __name__ == "__main__":          # the derivation of DEPTH_FIGURE: CPU only, a few minutes
    import time
    from oracle import oracle as O
    from path_tracer_amd import api, scenes
    O.build()
    t0 = time.time()
    sc = scenes.cornell_box(PG.E2E_W, PG.E2E_H)
    orc = O.Oracle(sc)
    r = api.Renderer(sc, PG.E2E_W, PG.E2E_H)
    grid = PG.oracle_probe_grid(orc, r, sc)
    far = two_rooms_max_distance(grid.cell)
    sums, counts = oracle_depth(orc, r, grid.nodes().reshape(-1, 3), PG.E2E_PROBE_SPP, E2E_RES, far)
    depth = Depth(means(sums, counts, far), E2E_FLOOR, E2E_FACING)
    print(f"oracle-baked grid and depth: {int(grid.valid.sum())} of {grid.valid.size} nodes valid, max_distance {far:.2f} ({time.time() - t0:.0f} s)")
    for name, dd in (("plain", None), ("depth", depth)):
        figure, signed, groups = PG.sh9_figure(orc, sc, grid) if dd is None else depth_figure(orc, sc, grid, dd)
        for model, (k, ga, gb) in groups.items():
            print(f"  {name} {model:14s} {k:5d} points: SH9 {ga / k:.5f}, cosine-sampled {gb / k:.5f}, {(ga - gb) / gb:+.4f}")
        print(f"{name}: figure = {figure:.4f} (signed difference of the sums {signed:+.4f}); the bound is {2 * figure:.4f} ({time.time() - t0:.0f} s)")
